// tests/fuseagg/fuseagg_plan_main.cpp -- drives duckdb-polr_amd/csrc/polr_fuseagg_plan.h alone, without a GPU
// (tests/test_fuseagg_plan.py writes the requests and checks the answers).
//
//   plan NAME has_out has_specs n_aggs already_fused      then one line per described aggregate, then "end":
//     agg fn src_join src_col col_in_range width flags
//   decode NAME n_aggs fn[n_aggs] word[1 + 3 n_aggs]      the combined cell table, words as unsigned decimals
//
// answers:  NAME code message / "  unfuse" or "  layout n_tables words cell_words has_sum", "  fn ..", "  kind ..", "  reset .."
//           decode NAME code message / "  value lo hi count is_null" per aggregate, or "  untouched 0|1" after a refusal
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../duckdb-polr_amd/csrc/polr_fuseagg_plan.h"

int main(int argc, char **argv) {
	if (argc != 2) {
		fprintf(stderr, "usage: %s requests.txt\n", argv[0]);
		return 2;
	}
	std::ifstream in(argv[1]);
	std::string line;
	unsigned n_done = 0;
	while (std::getline(in, line)) {
		std::istringstream ls(line);
		std::string what, name;
		ls >> what >> name;
		if (what == "plan") {
			int has_out, has_specs, already;
			uint32_t n_aggs;
			ls >> has_out >> has_specs >> n_aggs >> already;
			std::vector<PolrAggArg> args;
			while (std::getline(in, line) && line != "end") {
				std::istringstream as(line);
				std::string tag;
				PolrAggArg g; // (the column form: op = POLR_ARG_COLUMN, one operand)
				memset(&g, 0, sizeof(g));
				int in_range;
				as >> tag >> g.fn >> g.src_join[0] >> g.src_col[0] >> in_range >> g.col[0].width >> g.col[0].flags;
				g.col[0].in_range = in_range != 0;
				args.push_back(g);
			}
			PolrFuseAggRequest rq;
			memset(&rq, 0, sizeof(rq));
			rq.has_out = has_out != 0;
			rq.has_specs = has_specs != 0;
			rq.n_aggs = n_aggs;
			rq.already_fused = already != 0;
			rq.args = args.empty() ? nullptr : args.data(); // (a plan that reads what it was not given faults here)
			PolrFuseAggPlan pl;
			const int rc = polr_fuseagg_plan(rq, &pl);
			printf("%s %d %s\n", name.c_str(), rc, pl.err);
			if (rc == POLR_OK && pl.unfuse) {
				printf("  unfuse\n");
			} else if (rc == POLR_OK) {
				printf("  layout %u %u %" PRIu64 " %d\n", pl.n_tables, pl.words_per_table, pl.cell_words, pl.has_sum ? 1 : 0);
				printf("  fn");
				for (uint32_t a = 0; a < pl.n_aggs; a++) {
					printf(" %u", pl.fn[a]);
				}
				printf("\n  kind");
				for (uint32_t w = 0; w < pl.words_per_table; w++) {
					printf(" %u", (unsigned)pl.kind[w]);
				}
				printf("\n  reset");
				for (uint32_t w = 0; w < pl.words_per_table; w++) {
					printf(" %" PRIu64, pl.reset[w]);
				}
				printf("\n");
			}
		} else if (what == "decode") {
			uint32_t n_aggs;
			ls >> n_aggs;
			std::vector<uint32_t> fn(n_aggs);
			for (auto &f : fn) {
				ls >> f;
			}
			std::vector<uint64_t> cells(1u + 3u * n_aggs);
			for (auto &c : cells) {
				ls >> c;
			}
			std::vector<polr_agg_value> res(n_aggs);
			memset(res.data(), 0xA5, res.size() * sizeof(polr_agg_value));
			const std::vector<polr_agg_value> before = res;
			char err[256] = "";
			const int rc = polr_fuseagg_decode(fn.data(), n_aggs, cells.data(), res.data(), err, sizeof(err));
			printf("decode %s %d %s\n", name.c_str(), rc, err);
			if (rc == POLR_OK) {
				for (const auto &v : res) {
					printf("  value %" PRId64 " %" PRId64 " %" PRIu64 " %u\n", v.lo, v.hi, v.count, v.is_null);
				}
			} else {
				printf("  untouched %d\n", memcmp(res.data(), before.data(), res.size() * sizeof(polr_agg_value)) == 0 ? 1 : 0);
			}
		} else {
			continue;
		}
		n_done++;
	}
	printf("%u requests\nok\n", n_done);
	return 0;
}
