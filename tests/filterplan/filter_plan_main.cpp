// tests/filterplan/filter_plan_main.cpp -- duckdb-polr_amd/csrc/polr_filter_plan.h alone, as a stand-alone host program:
// reads filter programs from a text file, runs polr_filter_plan() on each and prints its verdict and, when the program is
// accepted, the lowered form.  tests/test_filter_plan.py writes the programs and checks the output.
//
//   filter_plan <file>
//     col <width> <signed>                       a probe column (before the first program; they apply to all)
//     program <name>
//     node <kind> <col> <op> <first_value> <n_values>
//     value <constant> <str_len> <-|x[hex]>      '-': str == NULL; 'x' + hex digits: the bytes (an allocation of exactly
//                                                their size)
//     counts <n_nodes> <n_values>                optional: the counts to pass instead of the lists' lengths
//     end
//   prints   <name> <code> [<message>]
//            and for code 0:  nodes / col / leaf / value / seg lines (see below)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../duckdb-polr_amd/csrc/polr_filter_plan.h"

int main(int argc, char **argv) {
	if (argc != 2) {
		fprintf(stderr, "usage: %s <programs file>\n", argv[0]);
		return 2;
	}
	FILE *f = fopen(argv[1], "r");
	if (!f) {
		perror(argv[1]);
		return 2;
	}
	std::vector<PolrFilterColumn> cols;
	std::vector<polr_filter_node> nodes;
	std::vector<polr_filter_value> values;
	std::vector<void *> owned;
	std::string name;
	long long n_nodes = -1, n_values = -1;
	static char line[20000], word[20000], hex[20000];
	unsigned programs = 0;
	while (fgets(line, sizeof(line), f)) {
		unsigned a, b, c, d, e;
		long long k;
		unsigned long long len;
		if (sscanf(line, "col %u %u", &a, &b) == 2) {
			cols.push_back(PolrFilterColumn{a, b});
		} else if (sscanf(line, "program %s", word) == 1) {
			name = word;
			nodes.clear();
			values.clear();
			n_nodes = n_values = -1;
		} else if (sscanf(line, "node %u %u %u %u %u", &a, &b, &c, &d, &e) == 5) {
			nodes.push_back(polr_filter_node{a, b, c, d, e, 0});
		} else if (sscanf(line, "value %lld %llu %s", &k, &len, hex) == 3) {
			polr_filter_value v = {k, nullptr, len};
			if (hex[0] == 'x') {
				const size_t n = (strlen(hex) - 1) / 2;
				uint8_t *p = (uint8_t *)malloc(n ? n : 1);
				for (size_t i = 0; i < n; i++) {
					unsigned byte = 0;
					sscanf(hex + 1 + 2 * i, "%2x", &byte);
					p[i] = (uint8_t)byte;
				}
				owned.push_back(p);
				v.str = p;
			}
			values.push_back(v);
		} else if (sscanf(line, "counts %lld %lld", &n_nodes, &n_values) == 2) {
		} else if (strncmp(line, "end", 3) == 0) {
			PolrFilterPlan pl;
			const int rc = polr_filter_plan(nodes.empty() ? nullptr : nodes.data(), n_nodes < 0 ? (uint32_t)nodes.size() : (uint32_t)n_nodes,
			                                values.empty() ? nullptr : values.data(),
			                                n_values < 0 ? (uint32_t)values.size() : (uint32_t)n_values, cols.data(), (uint32_t)cols.size(), pl);
			printf("%s %d %s\n", name.c_str(), rc, pl.err);
			programs++;
			if (rc == POLR_OK) {
				printf("  nodes");
				for (uint32_t i = 0; i < pl.n_nodes; i++) {
					printf(" %x", pl.nodes[i]);
				}
				printf("\n");
				for (uint32_t g = 0; g < pl.n_cols; g++) {
					printf("  col %u %u %u %u\n", pl.cols[g].col, pl.cols[g].first_leaf, pl.cols[g].n_leaves, pl.cols[g].needs_cell);
				}
				for (uint32_t l = 0; l < pl.n_leaves; l++) {
					printf("  leaf %u %u %u %u\n", pl.leaves[l].kind, pl.leaves[l].op, pl.leaves[l].first_value, pl.leaves[l].n_values);
				}
				for (size_t v = 0; v < pl.values.size(); v++) {
					const PolrFxValue &d = pl.values[v];
					printf("  value %lld %u %u pat %u %u %u %u\n", (long long)d.constant, d.c.len, d.bytes_off, d.pat.first_seg, d.pat.n_segs,
					       d.pat.flags, d.pat.min_len);
				}
				for (size_t s = 0; s < pl.segs.size(); s++) {
					printf("  seg %u %u\n", pl.segs[s].off, pl.segs[s].len);
				}
				printf("  bytes %zu\n", pl.bytes.size());
			}
			for (void *p : owned) {
				free(p);
			}
			owned.clear();
		}
	}
	fclose(f);
	printf("%u programs\nok\n", programs);
	return 0;
}
