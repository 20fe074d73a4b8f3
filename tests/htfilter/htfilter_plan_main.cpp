// tests/htfilter/htfilter_plan_main.cpp -- duckdb-polr_amd/csrc/polr_htfilter_plan.h alone, as a stand-alone host program:
// reads polr_ht_filter requests from a text file, runs polr_htfilter_plan() on each and prints its verdict and, when the
// request is accepted, the plan and the layout of the table's allocation for every kept count asked for.
// tests/test_htfilter_plan.py writes the requests and checks the output.
//
//   htfilter_plan <file>
//     request <name>
//     state <has_ht> <finalized> <filtered> <has_dict> <dict_col>
//     rows <n_rows>
//     key <width> <flags> <has_valid> <owned> <rebased>
//     payload <width> <flags> <has_valid> <owned> <rebased>
//     node <kind> <col> <op> <first_value> <n_values>
//     value <constant> <hex bytes | - for no string | = for an empty string>
//     counts <n_nodes> <n_values>          optional: the counts to pass instead of the lists' lengths
//     kept <n>                             any number: a layout is printed for each
//     end
//   prints   <name> <code> [<message>]
//            and for code 0:  number / fxcol / guard / scratch / layout / place lines (see below)
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../duckdb-polr_amd/csrc/polr_htfilter_plan.h"

int main(int argc, char **argv) {
	if (argc != 2) {
		fprintf(stderr, "usage: %s <requests file>\n", argv[0]);
		return 2;
	}
	FILE *f = fopen(argv[1], "r");
	if (!f) {
		perror(argv[1]);
		return 2;
	}
	std::vector<PolrHtFilterColumn> keys, payload;
	std::vector<polr_filter_node> nodes;
	std::vector<polr_filter_value> values;
	std::vector<std::string> strings; // the values' bytes
	std::vector<int> has_string;
	std::vector<unsigned long long> kept;
	PolrHtFilterRequest rq = {};
	std::string name;
	long long n_nodes = -1, n_values = -1;
	static char line[40000], word[40000];
	unsigned requests = 0;
	while (fgets(line, sizeof(line), f)) {
		unsigned a, b, c, d, e;
		unsigned long long r;
		long long k;
		if (sscanf(line, "request %s", word) == 1) {
			name = word;
			keys.clear();
			payload.clear();
			nodes.clear();
			values.clear();
			strings.clear();
			has_string.clear();
			kept.clear();
			rq = PolrHtFilterRequest();
			n_nodes = n_values = -1;
		} else if (sscanf(line, "state %u %u %u %u %u", &a, &b, &c, &d, &e) == 5) {
			rq.has_ht = a != 0;
			rq.finalized = b != 0;
			rq.filtered = c != 0;
			rq.has_dict = d != 0;
			rq.dict_col = e;
		} else if (sscanf(line, "rows %llu", &r) == 1) {
			rq.n_rows = r;
		} else if (sscanf(line, "key %u %u %u %u %u", &a, &b, &c, &d, &e) == 5) {
			keys.push_back(PolrHtFilterColumn{a, b, c, d, e});
		} else if (sscanf(line, "payload %u %u %u %u %u", &a, &b, &c, &d, &e) == 5) {
			payload.push_back(PolrHtFilterColumn{a, b, c, d, e});
		} else if (sscanf(line, "node %u %u %u %u %u", &a, &b, &c, &d, &e) == 5) {
			nodes.push_back(polr_filter_node{a, b, c, d, e, 0});
		} else if (sscanf(line, "value %lld %s", &k, word) == 2) {
			std::string s;
			if (word[0] != '-' && word[0] != '=') {
				for (size_t i = 0; word[i] && word[i + 1]; i += 2) {
					unsigned byte = 0;
					sscanf(word + i, "%2x", &byte);
					s.push_back((char)byte);
				}
			}
			strings.push_back(s);
			has_string.push_back(word[0] != '-');
			values.push_back(polr_filter_value{k, nullptr, 0});
		} else if (sscanf(line, "counts %lld %lld", &n_nodes, &n_values) == 2) {
		} else if (sscanf(line, "kept %llu", &r) == 1) {
			kept.push_back(r);
		} else if (strncmp(line, "end", 3) == 0) {
			for (size_t v = 0; v < values.size(); v++) { // (the strings no longer move)
				values[v].str = has_string[v] ? strings[v].data() : nullptr;
				values[v].str_len = strings[v].size();
			}
			rq.n_keys = (uint32_t)keys.size();
			rq.n_payload = (uint32_t)payload.size();
			rq.nodes = nodes.empty() ? nullptr : nodes.data();
			rq.values = values.empty() ? nullptr : values.data();
			rq.n_nodes = n_nodes < 0 ? (uint32_t)nodes.size() : (uint32_t)n_nodes;
			rq.n_values = n_values < 0 ? (uint32_t)values.size() : (uint32_t)n_values;
			// (exactly n_keys + n_payload entries: a plan that reads a column beyond them runs off the end under the address
			// sanitizer)
			std::vector<PolrHtFilterColumn> cols(keys);
			cols.insert(cols.end(), payload.begin(), payload.end());
			PolrHtFilterPlan pl;
			const int rc = polr_htfilter_plan(rq, cols.empty() ? nullptr : cols.data(), pl);
			printf("%s %d %s\n", name.c_str(), rc, pl.err);
			requests++;
			if (rc == POLR_OK) {
				for (uint32_t col = 0; col < cols.size(); col++) {
					uint32_t idx;
					const bool is_key = polr_htfilter_col(col, rq.n_keys, idx);
					printf("  number %u %d %u\n", col, is_key ? 1 : 0, idx);
				}
				for (uint32_t g = 0; g < pl.fx.n_cols; g++) {
					printf("  fxcol %u %u %u %u\n", pl.fx.cols[g].col, pl.fx.cols[g].first_leaf, pl.fx.cols[g].n_leaves, pl.fx.cols[g].needs_cell);
				}
				printf("  guard");
				for (uint32_t col : pl.guard) {
					printf(" %u", col);
				}
				printf("\n");
				printf("  scratch %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)pl.n_tiles, (unsigned long long)pl.n_words,
				       (unsigned long long)pl.bits_off, (unsigned long long)pl.base_off, (unsigned long long)pl.total_off,
				       (unsigned long long)pl.count_off, (unsigned long long)pl.scratch_bytes);
				for (unsigned long long n : kept) {
					PolrHtFilterLayout lo;
					polr_htfilter_layout(cols.data(), (uint32_t)cols.size(), n, lo);
					printf("  layout %llu %llu %llu %llu %zu\n", n, (unsigned long long)lo.table_bytes, (unsigned long long)lo.rows_off,
					       (unsigned long long)lo.desc_off, sizeof(PolrHtFilterDesc));
					for (size_t col = 0; col < cols.size(); col++) {
						printf("  place %llu %zu %llu %lld\n", n, col, (unsigned long long)lo.data_off[col],
						       lo.valid_off[col] == POLR_HTFILTER_NO_ARRAY ? -1ll : (long long)lo.valid_off[col]);
					}
				}
			}
		}
	}
	fclose(f);
	printf("%u requests\nok\n", requests);
	return 0;
}
