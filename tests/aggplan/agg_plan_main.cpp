// tests/aggplan/agg_plan_main.cpp -- drives duckdb-polr_amd/csrc/polr_agg_plan.h alone, without a GPU
// (tests/test_agg_plan.py writes the requests and checks the answers).
//
//   plan FAMILY NAME has_out has_keys has_specs has_results has_group_outputs agg_cells n_keys n_aggs n_groups max_groups
//        strings has_str_used has_str_bytes str_cap flat_emit already_fused
//     FAMILY: ungrouped | grouped | hashed | fuse; then one line per described group column and aggregate, then "end":
//       key src_join src_col n_values in_range width flags
//       agg fn op src_join0 src_col0 src_join1 src_col1 result_width result_flags in_range0 width0 flags0 in_range1 width1 flags1
//   arg NAME index <the fields of an agg line>            the argument rule alone
//   layout NAME capacity max_groups n_cols n_aggs strings cell_bytes counter_bytes
//   decode NAME fn sum_hi sum_lo mn mx count              the sum as a signed high and an unsigned low limb
//   words NAME n_aggs
//
// answers:  NAME code message / "  flags head_passed unfuse", and when accepted "  plan n_aggs n_groups str_mask" and
//           "  agg fn op lo hi" per aggregate;  "  offsets <the layout's twelve fields>";  "  value lo hi count is_null";
//           "  words n"
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../duckdb-polr_amd/csrc/polr_agg_plan.h"

static PolrAggCol read_col(std::istream &in) {
	PolrAggCol c;
	int in_range;
	in >> in_range >> c.width >> c.flags;
	c.in_range = in_range != 0;
	return c;
}

static PolrAggArg read_arg(std::istream &in) {
	PolrAggArg g;
	memset(&g, 0, sizeof(g));
	in >> g.fn >> g.op >> g.src_join[0] >> g.src_col[0] >> g.src_join[1] >> g.src_col[1] >> g.result_width >> g.result_flags;
	g.col[0] = read_col(in);
	g.col[1] = read_col(in);
	return g;
}

static void print_arg(const PolrAggArgPlan &ap) {
	printf("  agg %u %u %lld %lld\n", ap.fn, ap.op, ap.lo, ap.hi);
}

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
		ls >> what;
		if (what == "plan") {
			std::string family;
			int f[6], strings, has_str_used, has_str_bytes, flat_emit, already;
			PolrAggRequest rq;
			memset(&rq, 0, sizeof(rq));
			ls >> family >> name >> f[0] >> f[1] >> f[2] >> f[3] >> f[4] >> f[5] >> rq.n_keys >> rq.n_aggs >> rq.n_groups >> rq.max_groups >>
			    strings >> has_str_used >> has_str_bytes >> rq.str_cap >> flat_emit >> already;
			rq.has_out = f[0] != 0;
			rq.has_keys = f[1] != 0;
			rq.has_specs = f[2] != 0;
			rq.has_results = f[3] != 0;
			rq.has_group_outputs = f[4] != 0;
			rq.agg_cells = f[5] != 0;
			rq.strings = strings != 0;
			rq.has_str_used = has_str_used != 0;
			rq.has_str_bytes = has_str_bytes != 0;
			rq.flat_emit = flat_emit != 0;
			rq.already_fused = already != 0;
			std::vector<PolrAggGroupCol> keys;
			std::vector<PolrAggArg> args;
			while (std::getline(in, line) && line != "end") {
				std::istringstream as(line);
				std::string tag;
				as >> tag;
				if (tag == "key") {
					PolrAggGroupCol k;
					memset(&k, 0, sizeof(k));
					as >> k.src_join >> k.src_col >> k.n_values;
					k.col = read_col(as);
					keys.push_back(k);
				} else {
					args.push_back(read_arg(as));
				}
			}
			// (exact-size heap arrays: a plan that reads what it was not given is caught by the address sanitizer)
			rq.keys = keys.empty() ? nullptr : keys.data();
			rq.args = args.empty() ? nullptr : args.data();
			PolrAggPlan pl;
			const int rc = family == "ungrouped" ? polr_agg_plan_ungrouped(rq, &pl)
			               : family == "grouped" ? polr_agg_plan_grouped(rq, &pl)
			               : family == "hashed"  ? polr_agg_plan_hashed(rq, &pl)
			                                     : polr_agg_plan_fuse_grouped(rq, &pl);
			printf("%s %d %s\n", name.c_str(), rc, pl.err);
			printf("  flags %d %d\n", pl.head_passed ? 1 : 0, pl.unfuse ? 1 : 0);
			if (rc == POLR_OK && !pl.unfuse) {
				printf("  plan %u %" PRIu64 " %u\n", pl.n_aggs, pl.n_groups, pl.str_mask);
				for (uint32_t a = 0; a < pl.n_aggs; a++) {
					print_arg(pl.agg[a]);
				}
			}
		} else if (what == "arg") {
			uint32_t a;
			ls >> name >> a;
			const PolrAggArg g = read_arg(ls);
			PolrAggArgPlan ap;
			char err[256] = "";
			const int rc = polr_agg_arg_rule(g, a, &ap, err);
			printf("%s %d %s\n", name.c_str(), rc, err);
			if (rc == POLR_OK) {
				print_arg(ap);
			}
		} else if (what == "layout") {
			uint64_t capacity, max_groups, cell_bytes, counter_bytes;
			uint32_t n_cols, n_aggs;
			int strings;
			ls >> name >> capacity >> max_groups >> n_cols >> n_aggs >> strings >> cell_bytes >> counter_bytes;
			PolrHashAggLayout lo;
			polr_hashagg_layout(capacity, max_groups, n_cols, n_aggs, strings != 0, cell_bytes, counter_bytes, &lo);
			printf("%s 0 \n  offsets", name.c_str());
			for (uint64_t x : {lo.state, lo.nulls, lo.counters, lo.keys, lo.reps, lo.cells, lo.okeys, lo.oreps, lo.onulls, lo.ocells,
			                   lo.zero_bytes, lo.total}) {
				printf(" %" PRIu64, x);
			}
			printf("\n");
		} else if (what == "decode") {
			uint32_t fn;
			int64_t sum_hi;
			uint64_t sum_lo, count;
			long long mn, mx;
			ls >> name >> fn >> sum_hi >> sum_lo >> mn >> mx >> count;
			const __int128 sum = (__int128)(((unsigned __int128)(uint64_t)sum_hi << 64) | sum_lo);
			const polr_agg_value v = polr_agg_decode(fn, sum, mn, mx, count);
			printf("%s 0 \n  value %" PRId64 " %" PRId64 " %" PRIu64 " %u\n", name.c_str(), v.lo, v.hi, v.count, v.is_null);
		} else if (what == "words") {
			uint32_t n_aggs;
			ls >> name >> n_aggs;
			printf("%s 0 \n  words %u\n", name.c_str(), polr_fused_group_words(n_aggs));
		} else {
			continue;
		}
		n_done++;
	}
	printf("%u requests\nok\n", n_done);
	return 0;
}
