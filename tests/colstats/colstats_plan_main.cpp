// tests/colstats/colstats_plan_main.cpp -- duckdb-polr_amd/csrc/polr_colstats_plan.h alone, as a stand-alone host program:
// reads column-statistics requests from a text file, runs polr_colstats_plan() on each and prints its verdict and, when the
// request is accepted, the launch shape and the scratch; `finalize` lines go through the decision table of
// polr_ht_finalize_auto_stats, `info` lines through what polr_col_stats_plan_info reports.
// tests/test_colstats_plan.py writes the requests and checks the output.
//
//   colstats_plan <file>
//     request <name>
//     state <is_table> <has_handle> <has_cols> <has_stats> <finalized>
//     table <n_keys>
//     flags <flags> <selected>
//     rows <n_rows>
//     column <width> <flags> <data address>      one per column of the table / pipeline, in order
//     cols <c0> <c1> ...                          the columns named (at most 32 are read)
//     ncols <n>                                   optional: the count to pass instead of the list's length
//     end
//   prints   <name> <code> [<message>]
//            and for code 0:  "  launch <grid_x> <partials_off> <result_off> <record_bytes> <scratch_bytes>" and per named
//            column "  col <i> <column> <is_key> <idx> <cells_per_load> <tile_rows> <head_rows> <n_loads> <tail_rows> <n_tiles>
//            <grid> <stride_rows>"
//     finalize <name> <n_keys> <key_flags0> <key_flags1> <n_rows_in> <wants_stats> <n_valid> <min> <max> <signed>
//   prints   finalize <name> <needs_pass> <decision> <tries_perfect>
//     info <n_rows> <width>
//   prints   info <n_rows> <width> <cells_per_load> <loads_in_flight> <tile_rows> <n_workgroups> <stride_rows> <scratch_bytes>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../duckdb-polr_amd/csrc/polr_colstats_plan.h"

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
	std::vector<PolrColStatsColumn> columns;
	std::vector<uint32_t> cols;
	PolrColStatsRequest rq = {};
	std::string name;
	long long n_cols = -1;
	static char line[4096], word[4096];
	unsigned requests = 0;
	while (fgets(line, sizeof(line), f)) {
		unsigned a, b, c, d, e, g;
		unsigned long long r, q;
		long long mn, mx;
		if (sscanf(line, "request %s", word) == 1) {
			name = word;
			columns.clear();
			cols.clear();
			rq = PolrColStatsRequest();
			n_cols = -1;
		} else if (sscanf(line, "state %u %u %u %u %u", &a, &b, &c, &d, &e) == 5) {
			rq.is_table = a != 0;
			rq.who = rq.is_table ? "polr_ht_column_stats" : "polr_pipeline_column_stats";
			rq.has_handle = b != 0;
			rq.has_cols = c != 0;
			rq.has_stats = d != 0;
			rq.finalized = e != 0;
		} else if (sscanf(line, "table %u", &a) == 1) {
			rq.n_keys = a;
		} else if (sscanf(line, "flags %u %u", &a, &b) == 2) {
			rq.flags = a;
			rq.selected = b != 0;
		} else if (sscanf(line, "rows %llu", &r) == 1) {
			rq.n_rows = r;
		} else if (sscanf(line, "column %u %u %llu", &a, &b, &r) == 3) {
			columns.push_back(PolrColStatsColumn{a, b, r});
		} else if (strncmp(line, "cols", 4) == 0) {
			for (char *tok = strtok(line + 4, " \n"); tok; tok = strtok(nullptr, " \n")) {
				cols.push_back((uint32_t)strtoul(tok, nullptr, 10));
			}
		} else if (sscanf(line, "ncols %lld", &n_cols) == 1) {
		} else if (strncmp(line, "end", 3) == 0) {
			rq.n_columns = (uint32_t)columns.size();
			// (exactly as many entries as the lists hold: a plan that reads beyond them runs off the end under the address
			// sanitizer)
			static const uint32_t none[1] = {0}; // (an empty list that is not NULL: n_cols == 0 reads nothing of it)
			rq.cols = !rq.has_cols ? nullptr : cols.empty() ? none : cols.data();
			rq.n_cols = n_cols < 0 ? (uint32_t)cols.size() : (uint32_t)n_cols;
			PolrColStatsPlan pl;
			const int rc = polr_colstats_plan(rq, columns.empty() ? nullptr : columns.data(), pl);
			printf("%s %d %s\n", name.c_str(), rc, pl.err);
			requests++;
			if (rc == POLR_OK) {
				printf("  launch %u %llu %llu %llu %llu\n", pl.grid_x, (unsigned long long)pl.partials_off, (unsigned long long)pl.result_off,
				       (unsigned long long)pl.record_bytes, (unsigned long long)pl.scratch_bytes);
				for (uint32_t i = 0; i < pl.n_cols; i++) {
					const PolrColStatsShape &s = pl.shape[i];
					printf("  col %u %u %u %u %u %u %llu %llu %llu %llu %u %llu\n", i, rq.cols[i], pl.is_key[i], pl.idx[i], s.cells_per_load,
					       s.tile_rows, (unsigned long long)s.head_rows, (unsigned long long)s.n_loads, (unsigned long long)s.tail_rows,
					       (unsigned long long)s.n_tiles, s.grid, (unsigned long long)s.stride_rows);
				}
			}
		} else if (sscanf(line, "finalize %s %u %u %u %llu %u %llu %lld %lld %u", word, &a, &b, &c, &r, &d, &q, &mn, &mx, &g) == 10) {
			const uint32_t key_flags[POLR_MAX_KEYS] = {b, c, 0, 0};
			polr_col_stats st = polr_col_stats();
			st.n_valid = q;
			st.min_value = mn;
			st.max_value = mx;
			st.flags = g ? POLR_COL_SIGNED : 0;
			const bool pass = polr_colstats_finalize_needs_pass(a, key_flags, d != 0);
			bool tries = false;
			const PolrColStatsFinalize dec = polr_colstats_finalize(a, key_flags, r, pass, st, &tries);
			printf("finalize %s %d %d %d\n", word, pass ? 1 : 0, (int)dec, tries ? 1 : 0);
			requests++;
		} else if (sscanf(line, "info %llu %u", &r, &a) == 2) {
			PolrColStatsShape s;
			polr_colstats_shape(r, a, 0, false, POLR_COLSTATS_GRID_CAP, s);
			const uint64_t scratch = s.grid ? polr_build_buffer_bytes(((uint64_t)s.grid + 1) * POLR_COLSTATS_WORDS * 8) : 0;
			printf("info %llu %u %u %u %u %u %llu %llu\n", r, a, s.cells_per_load, POLR_COLSTATS_LOADS, s.tile_rows, s.grid,
			       (unsigned long long)s.stride_rows, (unsigned long long)scratch);
			requests++;
		}
	}
	fclose(f);
	printf("%u requests\nok\n", requests);
	return 0;
}
