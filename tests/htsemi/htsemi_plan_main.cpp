// tests/htsemi/htsemi_plan_main.cpp -- duckdb-polr_amd/csrc/polr_htsemi_plan.h alone, as a stand-alone host program: reads
// polr_ht_semi_filter requests from a text file, runs polr_htsemi_plan() on each and prints its verdict and, when the
// request is accepted, the plan and the layout of the table's allocation for every kept count asked for.
// tests/test_htsemi_plan.py writes the requests and checks the output.
//
//   htsemi_plan <file>
//     request <name>
//     state <has_ht> <finalized> <filtered> <has_dict> <dict_col>
//     rows <n_rows>
//     key <width> <flags> <has_valid> <owned> <rebased>
//     payload <width> <flags> <has_valid> <owned> <rebased>
//     by <has_by> <finalized> <is_ht> <same_place> <kind> <key_signed> <device_bytes> <packed> <null_eq>   one per filter, then
//     bykey <width> <flags> <shift> <min> <range>                                                     its keys, then
//     filter <flags> <n_cols> <col0> <col1> <col2> <col3>
//     nfilters <n>                         optional: the count to pass instead of the list's length
//     nullfilters                          optional: pass filters = NULL
//     kept <n>                             any number: a layout is printed for each
//     end
//   prints   <name> <code> [<message>]
//            and for code 0:  order / filter / fkey / scratch / layout / place lines (see below)
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../duckdb-polr_amd/csrc/polr_htsemi_plan.h"

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
	std::vector<PolrHtSemiBy> bys;
	std::vector<polr_semi_filter> filters;
	std::vector<unsigned long long> kept;
	PolrHtSemiRequest rq = {};
	std::string name;
	long long n_filters = -1;
	bool null_filters = false;
	static char line[4096], word[4096];
	unsigned requests = 0;
	while (fgets(line, sizeof(line), f)) {
		unsigned a, b, c, d, e, g, h, i;
		unsigned long long r, q;
		long long k;
		if (sscanf(line, "request %s", word) == 1) {
			name = word;
			keys.clear();
			payload.clear();
			bys.clear();
			filters.clear();
			kept.clear();
			rq = PolrHtSemiRequest();
			n_filters = -1;
			null_filters = false;
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
		} else if (sscanf(line, "by %u %u %u %u %u %u %llu %u %u", &a, &b, &c, &d, &e, &g, &r, &h, &i) == 9) {
			PolrHtSemiBy by = PolrHtSemiBy();
			by.has_by = a != 0;
			by.finalized = b != 0;
			by.is_ht = c != 0;
			by.same_place = d != 0;
			by.kind = e;
			by.key_signed = g;
			by.device_bytes = r;
			by.pack.packed = h;
			by.pack.null_eq = i;
			bys.push_back(by);
		} else if (sscanf(line, "bykey %u %u %u %lld %llu", &a, &b, &c, &k, &q) == 5) {
			PolrHtSemiBy &by = bys.back();
			if (by.n_keys < POLR_NKEYS) {
				by.key_width[by.n_keys] = a;
				by.key_flags[by.n_keys] = b;
				by.pack.shift[by.n_keys] = c;
				by.pack.min[by.n_keys] = k;
				by.pack.range[by.n_keys] = q;
			}
			by.n_keys++;
		} else if (sscanf(line, "filter %u %u %u %u %u %u", &a, &b, &c, &d, &e, &g) == 6) {
			polr_semi_filter sf = {};
			sf.by = nullptr; // (never followed by the plan)
			sf.flags = a;
			sf.n_cols = b;
			sf.cols[0] = c;
			sf.cols[1] = d;
			sf.cols[2] = e;
			sf.cols[3] = g;
			filters.push_back(sf);
		} else if (sscanf(line, "nfilters %lld", &n_filters) == 1) {
		} else if (strncmp(line, "nullfilters", 11) == 0) {
			null_filters = true;
		} else if (sscanf(line, "kept %llu", &r) == 1) {
			kept.push_back(r);
		} else if (strncmp(line, "end", 3) == 0) {
			rq.n_keys = (uint32_t)keys.size();
			rq.n_payload = (uint32_t)payload.size();
			// (exactly as many entries as the lists hold: a plan that reads beyond them runs off the end under the address
			// sanitizer)
			rq.filters = null_filters || filters.empty() ? nullptr : filters.data();
			rq.by = bys.empty() ? nullptr : bys.data();
			rq.n_filters = n_filters < 0 ? (uint32_t)filters.size() : (uint32_t)n_filters;
			std::vector<PolrHtFilterColumn> cols(keys);
			cols.insert(cols.end(), payload.begin(), payload.end());
			PolrHtSemiPlan pl;
			const int rc = polr_htsemi_plan(rq, cols.empty() ? nullptr : cols.data(), pl);
			printf("%s %d %s\n", name.c_str(), rc, pl.err);
			requests++;
			if (rc == POLR_OK) {
				printf("  order");
				for (uint32_t x = 0; x < pl.n_filters; x++) {
					printf(" %u", pl.order[x]);
				}
				printf("\n");
				for (uint32_t x = 0; x < pl.n_filters; x++) {
					printf("  filter %u %u %u\n", x, pl.f[x].n_keys, pl.f[x].anti);
					for (uint32_t y = 0; y < pl.f[x].n_keys; y++) {
						const PolrHtSemiKey &key = pl.f[x].key[y];
						uint32_t idx;
						const bool is_key = polr_htfilter_col(key.col, rq.n_keys, idx);
						printf("  fkey %u %u %u %d %u %u %u %u %u %lld %llu\n", x, y, key.col, is_key ? 1 : 0, idx, key.width, key.sx, key.shift,
						       key.null_eq, (long long)key.min, (unsigned long long)key.range);
					}
				}
				const PolrHtFilterPlan &sc = pl.scratch;
				printf("  scratch %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)sc.n_tiles, (unsigned long long)sc.n_words,
				       (unsigned long long)sc.bits_off, (unsigned long long)sc.base_off, (unsigned long long)sc.total_off,
				       (unsigned long long)sc.count_off, (unsigned long long)sc.scratch_bytes);
				for (unsigned long long n : kept) {
					PolrHtSemiLayout sl;
					polr_htsemi_layout(cols.empty() ? nullptr : cols.data(), (uint32_t)cols.size(), pl.carried, n, sl);
					printf("  layout %llu %llu %llu %llu %llu %u %zu\n", n, (unsigned long long)sl.lo.table_bytes,
					       (unsigned long long)sl.lo.rows_off, (unsigned long long)sl.lo.desc_off, (unsigned long long)sl.list_off, sl.n_desc,
					       sizeof(PolrHtFilterDesc));
					for (size_t col = 0; col < sl.lo.data_off.size(); col++) {
						printf("  place %llu %zu %llu %lld\n", n, col, (unsigned long long)sl.lo.data_off[col],
						       sl.lo.valid_off[col] == POLR_HTFILTER_NO_ARRAY ? -1ll : (long long)sl.lo.valid_off[col]);
					}
				}
			}
		}
	}
	fclose(f);
	printf("%u requests\nok\n", requests);
	return 0;
}
