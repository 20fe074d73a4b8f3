// tests/pdictplan/pdict_plan_main.cpp -- duckdb-polr_amd/csrc/polr_pdict_plan.h alone (and polr_dict_plan.h beneath it), as a
// stand-alone host program: reads requests from a text file, one a line, runs the rule each names and prints one line per
// answer.  tests/test_pdict_plan.py writes the requests and checks the answers.
//
//   pdict_plan <file>
//     encode <flags> <probe_col> <n_probe_cols> <width> <encoded> <encoded_as> <is_code_col> <n_rows> <has_selection> <n_selected>
//                                                  -> <code> <capacity> <sorted> <null_invalid> <selected> <own_valid>
//                                                     <n_insert> <message>
//     outcome <hip error 0|1> <n_long> <full> <probe_col>
//                                                  -> <code> <message>        (the HIP error's text: "out of memory")
//     layout <capacity> <n_rows> <n_insert>        -> <rep> <hash> <state> <first_row> <code> <slot_of_row> <row_of_code>
//                                                     <block_sums> <scalars> <n_long> <total> <n_blocks>
//     build_layout <capacity> <n_rows>             -> the same twelve values, of polr_dict_layout (the build side's)
//     fetch <found> <code_col> <n_codes> <list 0|1> <n> <code>...
//                                                  -> <code> <message>
//   the values are decimal
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <sstream>
#include <string>
#include <vector>

#include "../../duckdb-polr_amd/csrc/polr_pdict_plan.h"

static void print_layout(const PolrDictLayout &lo) {
	const uint64_t v[] = {lo.rep, lo.hash, lo.state, lo.first_row, lo.code, lo.slot_of_row, lo.row_of_code, lo.block_sums,
	                      lo.scalars, lo.n_long, lo.total};
	for (uint64_t x : v) {
		printf("%llu ", (unsigned long long)x);
	}
	printf("%u\n", lo.n_blocks);
}

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
	static char line[4000];
	unsigned requests = 0;
	while (fgets(line, sizeof(line), f)) {
		std::istringstream in(line);
		std::string what;
		if (!(in >> what)) {
			continue;
		}
		requests++;
		if (what == "encode") {
			PolrPDictRequest rq = {};
			uint32_t encoded, is_code, has_sel;
			in >> rq.flags >> rq.probe_col >> rq.n_probe_cols >> rq.width >> encoded >> rq.encoded_as >> is_code >> rq.n_rows >> has_sel >>
			    rq.n_selected;
			rq.encoded = encoded != 0;
			rq.is_code_col = is_code != 0;
			rq.has_selection = has_sel != 0;
			PolrPDictPlan pl;
			const int rc = polr_pdict_plan_encode(rq, &pl);
			printf("%d %llu %d %d %d %d %llu %s\n", rc, (unsigned long long)pl.capacity, pl.sorted ? 1 : 0, pl.null_invalid ? 1 : 0,
			       pl.selected ? 1 : 0, pl.own_valid ? 1 : 0, (unsigned long long)pl.n_insert, pl.err);
		} else if (what == "outcome") {
			uint32_t hip, full, col;
			unsigned long long n_long;
			in >> hip >> n_long >> full >> col;
			PolrPDictPlan pl = PolrPDictPlan();
			const int rc = polr_pdict_plan_outcome(hip ? "out of memory" : nullptr, n_long, full != 0, col, &pl);
			printf("%d %s\n", rc, pl.err);
		} else if (what == "layout") {
			unsigned long long capacity, n, n_insert;
			in >> capacity >> n >> n_insert;
			PolrDictLayout lo;
			polr_pdict_layout(capacity, n, n_insert, &lo);
			print_layout(lo);
		} else if (what == "build_layout") {
			unsigned long long capacity, n;
			in >> capacity >> n;
			PolrDictLayout lo;
			polr_dict_layout(capacity, n, &lo);
			print_layout(lo);
		} else if (what == "fetch") {
			uint32_t found, code_col, n_codes, list;
			unsigned long long n;
			in >> found >> code_col >> n_codes >> list >> n;
			std::vector<uint32_t> codes;
			for (uint32_t c; in >> c;) {
				codes.push_back(c);
			}
			codes.shrink_to_fit();
			PolrPDictPlan pl = PolrPDictPlan();
			const int rc = polr_pdict_plan_fetch(found != 0, code_col, n_codes, list ? codes.data() : nullptr, n, &pl);
			printf("%d %s\n", rc, pl.err);
		} else {
			fprintf(stderr, "unknown request: %s", line);
			return 2;
		}
	}
	fclose(f);
	printf("%u requests\nok\n", requests);
	return 0;
}
