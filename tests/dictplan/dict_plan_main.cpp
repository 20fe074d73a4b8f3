// tests/dictplan/dict_plan_main.cpp -- duckdb-polr_amd/csrc/polr_dict_plan.h and polr_strrec_plan.h alone, as a stand-alone
// host program: reads requests from a text file, one a line, runs the rule each names and prints one line per answer.  tests/test_dict_plan.py writes the requests and checks the answers.
//
//   dict_plan <file>
//     encode <flags> <finalized> <payload_col> <n_payload> <width> <encoded> <encoded_as> <n_rows>
//                                                  -> <code> <capacity> <sorted> <null_invalid> <message>
//     outcome <hip error 0|1> <n_long> <full> <payload_col>
//                                                  -> <code> <message>        (the HIP error's text: "out of memory")
//     layout <capacity> <n_rows>                   -> <rep> <hash> <state> <first_row> <code> <slot_of_row> <row_of_code>
//                                                     <block_sums> <scalars> <n_long> <total> <n_blocks>
//     sort <n_codes>                               -> <ping> <pong> <rep_old> <rank> <total> <n_tiles> <n_merge_passes>
//     bytes <n_rows> <has_valid> <n_codes>         -> <device bytes>
//     fetch <found> <code_col> <n_codes> <list 0|1> <n> <code>...
//                                                  -> <code> <message>        (n: the length the call claims; the codes given
//                                                     are all the program holds: a rule that reads further runs off the end)
//     records <n_offsets> <str_cap> <n> (<length> | -)...
//                                                  -> <used> <fits 0|1> (<offset> | -)...     (-: an entry without a record)
//   the values are decimal
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <sstream>
#include <string>
#include <vector>

#include "../../duckdb-polr_amd/csrc/polr_dict_plan.h"
#include "../../duckdb-polr_amd/csrc/polr_strrec_plan.h"

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
			PolrDictRequest rq = {};
			uint32_t finalized, encoded;
			in >> rq.flags >> finalized >> rq.payload_col >> rq.n_payload >> rq.width >> encoded >> rq.encoded_as >> rq.n_rows;
			rq.finalized = finalized != 0;
			rq.encoded = encoded != 0;
			PolrDictPlan pl;
			const int rc = polr_dict_plan_encode(rq, &pl);
			printf("%d %llu %d %d %s\n", rc, (unsigned long long)pl.capacity, pl.sorted ? 1 : 0, pl.null_invalid ? 1 : 0, pl.err);
		} else if (what == "outcome") {
			uint32_t hip, full, col;
			unsigned long long n_long;
			in >> hip >> n_long >> full >> col;
			PolrDictPlan pl = {};
			const int rc = polr_dict_plan_outcome(hip ? "out of memory" : nullptr, n_long, full != 0, col, &pl);
			printf("%d %s\n", rc, pl.err);
		} else if (what == "layout") {
			unsigned long long capacity, n;
			in >> capacity >> n;
			PolrDictLayout lo;
			polr_dict_layout(capacity, n, &lo);
			const uint64_t v[] = {lo.rep, lo.hash, lo.state, lo.first_row, lo.code, lo.slot_of_row, lo.row_of_code, lo.block_sums,
			                      lo.scalars, lo.n_long, lo.total};
			for (uint64_t x : v) {
				printf("%llu ", (unsigned long long)x);
			}
			printf("%u\n", lo.n_blocks);
		} else if (what == "sort") {
			unsigned long long nc;
			in >> nc;
			PolrDictSortLayout so;
			polr_dict_sort_layout(nc, &so);
			printf("%llu %llu %llu %llu %llu %u %u\n", (unsigned long long)so.ping, (unsigned long long)so.pong,
			       (unsigned long long)so.rep_old, (unsigned long long)so.rank, (unsigned long long)so.total, so.n_tiles, so.n_merge_passes);
		} else if (what == "bytes") {
			unsigned long long n;
			uint32_t has_valid, nc;
			in >> n >> has_valid >> nc;
			printf("%llu\n", (unsigned long long)polr_dict_device_bytes(n, has_valid != 0, nc));
		} else if (what == "fetch") {
			uint32_t found, code_col, n_codes, list;
			unsigned long long n;
			in >> found >> code_col >> n_codes >> list >> n;
			std::vector<uint32_t> codes;
			for (uint32_t c; in >> c;) {
				codes.push_back(c);
			}
			codes.shrink_to_fit();
			PolrDictPlan pl = {};
			const int rc = polr_dict_plan_fetch(found != 0, code_col, n_codes, list ? codes.data() : nullptr, n, &pl);
			printf("%d %s\n", rc, pl.err);
		} else if (what == "records") {
			unsigned long long n_offsets, cap, n;
			in >> n_offsets >> cap >> n;
			std::vector<uint32_t> lens(n);
			std::vector<uint8_t> skip(n);
			std::vector<uint64_t> offs(n);
			for (uint64_t i = 0; i < n; i++) {
				std::string w;
				in >> w;
				skip[i] = w == "-";
				lens[i] = skip[i] ? 0xDEADBEEFu : (uint32_t)std::stoull(w); // (the length of an entry without a record is not read)
			}
			uint64_t calls = 0; // (the rule asks for every entry once, in order)
			const uint64_t used = polr_strrec_layout(n, [&](uint64_t i) {
				if (i != calls++) {
					fprintf(stderr, "entry %llu asked out of order: %s", (unsigned long long)i, line);
					exit(1);
				}
				return skip[i] ? POLR_STRREC_NONE : (uint64_t)lens[i];
			}, offs.data());
			if (calls != n) {
				fprintf(stderr, "%llu entries asked of %llu: %s", (unsigned long long)calls, n, line);
				return 1;
			}
			printf("%llu %d", (unsigned long long)used, polr_strrec_fits(used, cap, n, n_offsets) ? 1 : 0);
			for (uint64_t i = 0; i < n; i++) {
				if (offs[i] == POLR_STRREC_NONE) {
					printf(" -");
				} else {
					printf(" %llu", (unsigned long long)offs[i]);
				}
			}
			printf("\n");
		} else {
			fprintf(stderr, "unknown request: %s", line);
			return 2;
		}
	}
	fclose(f);
	printf("%u requests\nok\n", requests);
	return 0;
}
