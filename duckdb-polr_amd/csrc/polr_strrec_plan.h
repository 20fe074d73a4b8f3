// duckdb-polr_amd/csrc/polr_strrec_plan.h -- the string records by which strings leave the device, as plain host code: the
// one format behind polr_ht_fetch_dictionary, polr_ht_fetch_dictionary_codes and polr_out_aggregate_hashed_str / _expr
// (include/polr_hip.h).  No HIP in here: the three callers lay their records out with polr_strrec_layout and hand the
// offsets to polr_fetch_str_records (polr_strheap.hip), which checks the capacity rule, launches and copies;
// tests/dictplan/dict_plan_main.cpp drives the header alone.
//
// A record is {uint32 length, little endian; the string's bytes}, nothing between two records, no padding.  The host knows
// every length before a byte is written, so it lays the records out: entry i of a list gets the offset at which the
// records before it end, or no record at all (a NULL group value, an integer group column).  Nothing is written unless
// everything fits: the caller learns the exact size and calls again.
#pragma once

#include <stdint.h>

#define POLR_STRREC_NONE 0xFFFFFFFFFFFFFFFFull // the offset of an entry without a record, and its "length"

// len_of(i): the length of entry i's string, or POLR_STRREC_NONE for an entry without a record; called once per entry,
// i = 0 .. n - 1 in this order.
// -> offsets[n], and the bytes all records take (64-bit: 2^30 strings of 4 GB do not wrap)
template <class LenOf>
static inline uint64_t polr_strrec_layout(uint64_t n, LenOf len_of, uint64_t *offsets) {
	uint64_t used = 0;
	for (uint64_t i = 0; i < n; i++) {
		const uint64_t len = len_of(i);
		if (len == POLR_STRREC_NONE) {
			offsets[i] = POLR_STRREC_NONE;
			continue;
		}
		offsets[i] = used;
		used += 4ull + len;
	}
	return used;
}

// the capacity rule (POLR_E_OVERFLOW otherwise, *str_used exact, nothing written): the arena holds all records and, where
// the call returns offsets, the caller made room for all n of them (no offsets returned: n_offsets = n)
static inline bool polr_strrec_fits(uint64_t used, uint64_t str_cap, uint64_t n, uint64_t n_offsets) {
	return used <= str_cap && n_offsets >= n;
}
