// tests/buildplan/build_plan_main.cpp -- duckdb-polr_amd/csrc/polr_build_plan.h alone, as a stand-alone host program:
// reads requests from a text file, one a line, runs the rule each names and prints one line per answer.
// tests/test_build_plan.py writes the requests and checks the answers.
//
//   build_plan <file>
//     rows <n_rows>                                              -> <code> <message>
//     colwidth <width>                                           -> <code> <message>
//     keys <n_keys> <width>...                                   -> <code> <message>
//     layout <row_width> <n_cols> (<offset> <width>)...          -> <code> <message>
//     perfect <min> <max> <signed>                               -> <code> <range> <size> <words> <message>
//     pht <key_width> <min> <max> <signed>                       -> <code> <range> <size> <words> <message>
//     auto <n_rows_in> <min> <max> <signed> <n_keys> <flags>...  -> <0|1>
//     capacity <n>                                               -> <code> <capacity> <message>
//     needs_pack <n_keys> (<width> <flags>)...                   -> <0|1>
//     kind <longest_run> <sentinels> <n_keys> <width0> <packed>  -> <code> <kind> <max_run> <message>
//     pack <n_keys> <null_eq> (<min> <max> <col_flags>)...       -> <code> <packed> <null_eq> (<shift> <sx> <min> <range>)... | <message>
//     buffers <kind> <capacity> <n_rows_in> <n_payload> (<width> <has_valid>)...
//                                                                -> <n> (<what> <col> <bytes>)...   the list export reports
//                                                                   <n> (<what> <col> <bytes>)...   ... and alloc_like allocates
//     meta <kind> <n_keys> <n_payload> <capacity> <range> <n_rows_in> <magic> <key_width0> <payload_width0>
//                                                                -> <code> <message>
//   the values are decimal; <min> and <max> are signed 64-bit (an unsigned key's bit pattern)
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "../../duckdb-polr_amd/csrc/polr_build_plan.h"

static void print_buffers(const std::vector<PolrBuildBuffer> &bufs) {
	printf("%zu", bufs.size());
	for (const PolrBuildBuffer &b : bufs) {
		printf(" %u %u %llu", b.what, b.col, (unsigned long long)b.bytes);
	}
	printf("\n");
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
		if (what == "rows") {
			unsigned long long n;
			in >> n;
			PolrBuildPlan pl;
			const int rc = polr_build_check_rows(n, pl);
			printf("%d %s\n", rc, pl.err);
		} else if (what == "colwidth") {
			uint32_t w;
			in >> w;
			PolrBuildPlan pl;
			const int rc = polr_build_check_col_width(w, pl);
			printf("%d %s\n", rc, pl.err);
		} else if (what == "keys") {
			size_t n;
			in >> n;
			std::vector<uint32_t> w; // (exactly the widths given: a check that reads past them runs off the end)
			for (uint32_t x; in >> x;) {
				w.push_back(x);
			}
			PolrBuildPlan pl;
			const int rc = polr_build_check_keys(n, w.data(), pl);
			printf("%d %s\n", rc, pl.err);
		} else if (what == "layout") {
			uint32_t row_width, n;
			in >> row_width >> n;
			std::vector<uint32_t> off(n), w(n);
			for (uint32_t c = 0; c < n; c++) {
				in >> off[c] >> w[c];
			}
			PolrBuildPlan pl;
			const int rc = polr_build_check_row_layout(row_width, n, off.data(), w.data(), pl);
			printf("%d %s\n", rc, pl.err);
		} else if (what == "perfect" || what == "pht") {
			uint32_t key_width = 4, is_signed;
			long long mn, mx;
			if (what == "pht") {
				in >> key_width;
			}
			in >> mn >> mx >> is_signed;
			PolrPerfectPlan pl;
			const int rc = what == "pht" ? polr_build_pht_upload(key_width, mn, mx, is_signed != 0, pl)
			                             : polr_build_perfect_range(mn, mx, is_signed != 0, pl);
			printf("%d %llu %llu %llu %s\n", rc, (unsigned long long)pl.range, (unsigned long long)pl.size,
			       (unsigned long long)pl.words, pl.err);
		} else if (what == "auto") {
			unsigned long long n;
			long long mn, mx;
			uint32_t is_signed, n_keys;
			in >> n >> mn >> mx >> is_signed >> n_keys;
			std::vector<uint32_t> flags(n_keys);
			for (uint32_t c = 0; c < n_keys; c++) {
				in >> flags[c];
			}
			printf("%d\n", polr_build_auto_tries_perfect(n_keys, flags.data(), n, mn, mx, is_signed != 0) ? 1 : 0);
		} else if (what == "capacity") {
			unsigned long long n;
			in >> n;
			PolrCapacityPlan pl;
			const int rc = polr_build_capacity(n, pl);
			printf("%d %llu %s\n", rc, (unsigned long long)pl.capacity, pl.err);
		} else if (what == "needs_pack") {
			uint32_t n_keys;
			in >> n_keys;
			std::vector<uint32_t> w(n_keys), flags(n_keys);
			for (uint32_t c = 0; c < n_keys; c++) {
				in >> w[c] >> flags[c];
			}
			printf("%d\n", polr_build_needs_key_pack(n_keys, w.data(), flags.data()) ? 1 : 0);
		} else if (what == "kind") {
			unsigned long long run, sentinels;
			uint32_t n_keys, w0, packed;
			in >> run >> sentinels >> n_keys >> w0 >> packed;
			PolrKindPlan pl;
			const int rc = polr_build_hash_kind(run, sentinels, n_keys, w0, packed != 0, pl);
			printf("%d %u %llu %s\n", rc, pl.kind, (unsigned long long)pl.max_run, pl.err);
		} else if (what == "pack") {
			uint32_t n_keys, null_eq;
			in >> n_keys >> null_eq;
			std::vector<long long> mm(2 * n_keys);
			std::vector<uint32_t> flags(n_keys);
			for (uint32_t c = 0; c < n_keys; c++) {
				in >> mm[2 * c] >> mm[2 * c + 1] >> flags[c];
			}
			PolrKeyPackPlan pl;
			const int rc = polr_build_key_pack(n_keys, mm.data(), null_eq, flags.data(), pl);
			printf("%d", rc);
			if (rc == POLR_OK) {
				printf(" %u %u", pl.pack.packed, pl.pack.null_eq);
				for (uint32_t c = 0; c < n_keys; c++) {
					printf(" %u %u %lld %llu", pl.pack.shift[c], pl.pack.sx[c], (long long)pl.pack.min[c],
					       (unsigned long long)pl.pack.range[c]);
				}
				printf("\n");
			} else {
				printf(" %s\n", pl.err);
			}
		} else if (what == "buffers") {
			// the sending side lists the buffers of the table it describes; the receiving side those of the blob it got
			PolrHtMeta m;
			memset(&m, 0, sizeof(m));
			in >> m.kind >> m.capacity >> m.n_rows_in >> m.n_payload;
			std::vector<uint32_t> w(m.n_payload);
			std::vector<uint8_t> has_valid(m.n_payload);
			for (uint32_t i = 0; i < m.n_payload; i++) {
				uint32_t v;
				in >> w[i] >> v;
				has_valid[i] = v ? 1 : 0;
				m.payload_width[i] = w[i];
				m.payload_has_valid[i] = has_valid[i];
			}
			std::vector<PolrBuildBuffer> sent, received;
			polr_build_buffers(m.kind, m.capacity, m.n_rows_in, m.n_payload, w.data(), has_valid.data(), sent);
			static char blob[sizeof(PolrHtMeta)];
			memcpy(blob, &m, sizeof(m));
			PolrHtMeta got;
			memcpy(&got, blob, sizeof(got));
			polr_build_buffers(got.kind, got.capacity, got.n_rows_in, got.n_payload, got.payload_width, got.payload_has_valid,
			                   received);
			print_buffers(sent);
			print_buffers(received);
		} else if (what == "meta") {
			PolrHtMeta m;
			memset(&m, 0, sizeof(m));
			in >> m.kind >> m.n_keys >> m.n_payload >> m.capacity >> m.range >> m.n_rows_in >> m.magic;
			uint32_t kw, pw;
			in >> kw >> pw;
			for (uint32_t i = 0; i < POLR_MAX_KEYS; i++) {
				m.key_width[i] = i == 0 ? kw : 4;
			}
			for (uint32_t i = 0; i < POLR_BUILD_MAX_PAYLOAD; i++) {
				m.payload_width[i] = i == 0 ? pw : 8;
			}
			PolrBuildPlan pl;
			const int rc = polr_build_check_meta(m, pl);
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
