// tests/fromout/fromout_plan_main.cpp -- duckdb-polr_amd/csrc/polr_fromout_plan.h alone, as a stand-alone host program:
// reads polr_ht_from_output requests from a text file, runs polr_fromout_plan() on each and prints its verdict and, when
// the request is accepted, the plan.  tests/test_fromout_plan.py writes the requests and checks the output.
//
//   fromout_plan <file>
//     request <name>
//     flags <has_out> <has_result> <has_keys> <has_payload> <fused>
//     rows <n_rows> <n_chunks>
//     key <resolved> <slot> <width> <flags> <has_valid> <owned> <rebased>
//     payload <resolved> <slot> <width> <flags> <has_valid> <owned> <rebased>
//     counts <n_keys> <n_payload>                optional: the counts to pass instead of the lists' lengths
//     end
//   prints   <name> <code> [<message>]
//            and for code 0:  fixed / string / slots / bytes / place / scratch lines (see below)
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../duckdb-polr_amd/csrc/polr_fromout_plan.h"

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
	std::vector<PolrFromoutColumn> keys, payload;
	PolrFromoutRequest rq = {};
	std::string name;
	long long n_keys = -1, n_payload = -1;
	static char line[1000], word[1000];
	unsigned requests = 0;
	while (fgets(line, sizeof(line), f)) {
		unsigned a, b, c, d, e, g, h;
		unsigned long long r, nc;
		if (sscanf(line, "request %s", word) == 1) {
			name = word;
			keys.clear();
			payload.clear();
			rq = PolrFromoutRequest();
			n_keys = n_payload = -1;
		} else if (sscanf(line, "flags %u %u %u %u %u", &a, &b, &c, &d, &e) == 5) {
			rq.has_out = a != 0;
			rq.has_result = b != 0;
			rq.has_keys = c != 0;
			rq.has_payload = d != 0;
			rq.fused = e != 0;
		} else if (sscanf(line, "rows %llu %llu", &r, &nc) == 2) {
			rq.n_rows = r;
			rq.n_chunks = nc;
		} else if (sscanf(line, "key %u %u %u %u %u %u %u", &a, &b, &c, &d, &e, &g, &h) == 7) {
			keys.push_back(PolrFromoutColumn{a, b, c, d, e, g, h});
		} else if (sscanf(line, "payload %u %u %u %u %u %u %u", &a, &b, &c, &d, &e, &g, &h) == 7) {
			payload.push_back(PolrFromoutColumn{a, b, c, d, e, g, h});
		} else if (sscanf(line, "counts %lld %lld", &n_keys, &n_payload) == 2) {
		} else if (strncmp(line, "end", 3) == 0) {
			rq.n_keys = n_keys < 0 ? (uint32_t)keys.size() : (uint32_t)n_keys;
			rq.n_payload = n_payload < 0 ? (uint32_t)payload.size() : (uint32_t)n_payload;
			// (the array as the library passes it: exactly n_keys + n_payload entries, so that a plan that reads a column it
			// should have refused the request before runs off its end under the address sanitizer)
			std::vector<PolrFromoutColumn> cols;
			if (rq.has_keys && rq.n_keys <= keys.size() && (rq.has_payload || rq.n_payload == 0) && rq.n_payload <= payload.size()) {
				cols.insert(cols.end(), keys.begin(), keys.begin() + rq.n_keys);
				cols.insert(cols.end(), payload.begin(), payload.begin() + rq.n_payload);
			}
			PolrFromoutPlan pl;
			const int rc = polr_fromout_plan(rq, cols.empty() ? nullptr : cols.data(), pl);
			printf("%s %d %s\n", name.c_str(), rc, pl.err);
			requests++;
			if (rc == POLR_OK) {
				for (const PolrFromoutFixed &x : pl.fixed) {
					printf("  fixed %u %u %u\n", x.col, x.slot, x.width);
				}
				for (const PolrFromoutString &x : pl.strings) {
					printf("  string %u %u %u\n", x.col, x.slot, x.needs_heap_guard);
				}
				printf("  slots %u", pl.n_slots);
				for (uint32_t g = 0; g <= pl.n_slots; g++) {
					printf(" %u", pl.group_first[g]);
				}
				printf("\n");
				printf("  bytes %llu %llu %zu\n", (unsigned long long)pl.table_bytes, (unsigned long long)pl.desc_off, sizeof(PolrFromoutDesc));
				for (size_t c = 0; c < pl.data_off.size(); c++) {
					printf("  place %llu %llu\n", (unsigned long long)pl.data_off[c], (unsigned long long)pl.valid_off[c]);
				}
				printf("  scratch %llu %llu %llu\n", (unsigned long long)pl.row_off_words, (unsigned long long)pl.chunk_words,
				       (unsigned long long)pl.tail_words);
			}
		}
	}
	fclose(f);
	printf("%u requests\nok\n", requests);
	return 0;
}
