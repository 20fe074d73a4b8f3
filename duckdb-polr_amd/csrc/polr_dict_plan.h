// duckdb-polr_amd/csrc/polr_dict_plan.h -- the host rules of the dictionary of a VARCHAR build column
// (polr_ht_encode_dictionary[_ex], polr_ht_fetch_dictionary[_codes]; include/polr_hip.h), as plain host code.  No HIP in
// here: polr_dict.hip describes the request, asks the plan, and allocates and launches what the plan says; the strings
// leave the device as the records of polr_strrec_plan.h; a stand-alone host program drives the header alone
// (tests/dictplan/dict_plan_main.cpp).
//
// Every refusal, in this order, each with its message:
//
//   polr_dict_plan_encode        polr_ht_encode_dictionary, polr_ht_encode_dictionary_ex
//     1. a flag other than POLR_DICT_SORTED and POLR_DICT_NULL_INVALID        POLR_E_INVALID
//     2. the table is finalized already                                       POLR_E_INVALID
//     3. no such payload column                                               POLR_E_INVALID
//     4. not a column of 16-byte string cells                                 POLR_E_INVALID
//     5. the column is encoded already (names its code column)                POLR_E_INVALID
//     6. the table has POLR_BUILD_MAX_PAYLOAD payload columns already         POLR_E_UNSUPPORTED
//     7. the string table's slots exceed the 32-bit slot space                POLR_E_UNSUPPORTED
//
//   polr_dict_plan_outcome       ... once the device has answered
//     1. a HIP error                                                          POLR_E_HIP
//     2. strings longer than 12 bytes, but the column's heap never came       POLR_E_INVALID
//     3. the string table filled up (capacity >= 2 x rows: cannot happen)     POLR_E_HIP
//
//   polr_dict_plan_fetch         polr_ht_fetch_dictionary, polr_ht_fetch_dictionary_codes
//     1. not a code column whose dictionary the table holds                   POLR_E_INVALID
//     2. (a code list) more than 2^30 listed codes                            POLR_E_UNSUPPORTED
//     3. (a code list) a listed code >= n_codes, the first such position      POLR_E_INVALID
//
// Besides: polr_dict_layout (the encoder's one scratch allocation), polr_dict_sort_layout (the scratch of the sort of n_codes
// values) and polr_dict_device_bytes (what an encoded column adds to the table's device bytes).
#pragma once

#include <stdint.h>
#include <stdio.h>

#include "../../include/polr_hip.h"
#include "polr_build_plan.h" // polr_build_capacity, polr_build_buffer_bytes, POLR_BUILD_MAX_PAYLOAD

#define POLR_DICT_BLOCK 256u
#define POLR_DICT_ITEMS 4u         // rows per thread of the rank step: 1024 rows per workgroup
#define POLR_DICT_SORT_TILE 1024u  // records a workgroup sorts or merges in LDS: 16 KB of the CU's 160
#define POLR_DICT_REC_BYTES 16u    // a sort record (DictRec, polr_dict.hip)
#define POLR_DICT_MAX_LIST (1ull << 30) // codes one polr_ht_fetch_dictionary_codes call lists

struct PolrDictRequest {
	uint32_t flags, payload_col;
	bool finalized;      // the table's kind is set
	uint32_t n_payload;
	uint32_t width;      // of the payload column (read where payload_col < n_payload)
	bool encoded;        // a dictionary of this column exists ...
	uint32_t encoded_as; // ... and this is its code column
	uint64_t n_rows;     // build rows as uploaded
};
struct PolrDictPlan {
	char err[256];
	bool sorted, null_invalid;
	uint64_t capacity; // slots of the string table
};

#define POLR_DP_REFUSE(code_, ...)                                                                                     \
	do {                                                                                                               \
		snprintf(pl->err, sizeof(pl->err), __VA_ARGS__);                                                               \
		return (code_);                                                                                                \
	} while (0)

static inline int polr_dict_plan_encode(const PolrDictRequest &rq, PolrDictPlan *pl) {
	*pl = PolrDictPlan();
	if (rq.flags & ~(POLR_DICT_SORTED | POLR_DICT_NULL_INVALID)) {
		POLR_DP_REFUSE(POLR_E_INVALID, "dictionary flags 0x%x: only POLR_DICT_SORTED and POLR_DICT_NULL_INVALID are defined", rq.flags);
	}
	pl->sorted = (rq.flags & POLR_DICT_SORTED) != 0;
	pl->null_invalid = (rq.flags & POLR_DICT_NULL_INVALID) != 0;
	if (rq.finalized) {
		// (a finalized perfect table keeps a re-ordered copy of every payload column, and the engines hold the column array)
		POLR_DP_REFUSE(POLR_E_INVALID, "a payload column is dictionary-encoded before the table is finalized");
	}
	if (rq.payload_col >= rq.n_payload) {
		POLR_DP_REFUSE(POLR_E_INVALID, "payload column %u of %u", rq.payload_col, rq.n_payload);
	}
	if (rq.width != 16) {
		POLR_DP_REFUSE(POLR_E_INVALID, "a dictionary is made of a column of 16-byte string cells (this one: %u bytes)", rq.width);
	}
	if (rq.encoded) {
		POLR_DP_REFUSE(POLR_E_INVALID, "payload column %u is encoded already (code column %u)", rq.payload_col, rq.encoded_as);
	}
	if (rq.n_payload >= POLR_BUILD_MAX_PAYLOAD) {
		// (polr_ht_export / polr_ht_alloc_like describe no more payload columns: no table is made that cannot be shipped)
		POLR_DP_REFUSE(POLR_E_UNSUPPORTED, "the table has %u payload columns already: a code column would be the %urd, more than "
		                                   "polr_ht_export carries", rq.n_payload, POLR_BUILD_MAX_PAYLOAD + 1);
	}
	PolrCapacityPlan slots; // the string table: a slot space of its own, the build side's capacity rule
	if (polr_build_capacity(rq.n_rows, slots)) {
		POLR_DP_REFUSE(POLR_E_UNSUPPORTED, "a dictionary over %llu build rows exceeds the 32-bit slot space", (unsigned long long)rq.n_rows);
	}
	pl->capacity = slots.capacity;
	return POLR_OK;
}

// hip_error: the text of the HIP error of the read-back, or NULL; n_long: the heap guard's count; full: the table's flag
static inline int polr_dict_plan_outcome(const char *hip_error, unsigned long long n_long, bool full, uint32_t payload_col,
                                         PolrDictPlan *pl) {
	if (hip_error) {
		POLR_DP_REFUSE(POLR_E_HIP, "dictionary encoding failed: %s", hip_error);
	}
	if (n_long) {
		POLR_DP_REFUSE(POLR_E_INVALID,
		               "payload column %u: %llu build rows hold strings longer than 12 bytes, but the column's heap was never put on the "
		               "device (polr_ht_set_payload_heaps)",
		               payload_col, n_long);
	}
	if (full) {
		POLR_DP_REFUSE(POLR_E_HIP, "dictionary encoding failed: the string table filled up");
	}
	return POLR_OK;
}

// found: the table holds a dictionary whose code column is code_col, of n_codes strings.  codes = NULL: the whole
// dictionary; else the list of n codes (read only where the rules before it passed)
static inline int polr_dict_plan_fetch(bool found, uint32_t code_col, uint32_t n_codes, const uint32_t *codes, uint64_t n,
                                       PolrDictPlan *pl) {
	if (!found) {
		// (also a table made by polr_ht_alloc_like / received by polr_bcast_build: it carries the codes, not the strings)
		POLR_DP_REFUSE(POLR_E_INVALID, "payload column %u is not a code column whose dictionary this table holds", code_col);
	}
	if (!codes) {
		return POLR_OK;
	}
	if (n > POLR_DICT_MAX_LIST) {
		POLR_DP_REFUSE(POLR_E_UNSUPPORTED, "a list of %llu codes: at most 2^30 strings are fetched by one call", (unsigned long long)n);
	}
	for (uint64_t i = 0; i < n; i++) {
		if (codes[i] >= n_codes) { // (nothing was written, *str_used included)
			POLR_DP_REFUSE(POLR_E_INVALID, "code %u at position %llu of the list: the dictionary has %u strings (the NULL code is none)",
			               codes[i], (unsigned long long)i, n_codes);
		}
	}
	return POLR_OK;
}

// The encoder's single scratch allocation, as byte offsets: the string table (representative cells, hashes, states, first
// rows, codes: `capacity` entries each), the per-row arrays and the block sums of the rank step (each rounded up to 16
// bytes), and 64 bytes of scalars -- the heap guard's 64-bit count sits 32 bytes into them.
struct PolrDictLayout {
	uint64_t rep, hash, state, first_row, code, slot_of_row, row_of_code, block_sums, scalars, n_long;
	uint64_t total;
	uint32_t n_blocks; // workgroups of the rank step: POLR_DICT_BLOCK * POLR_DICT_ITEMS rows each, at least one
};
static inline void polr_dict_layout(uint64_t capacity, uint64_t n_rows, PolrDictLayout *lo) {
	const uint64_t per_block = POLR_DICT_BLOCK * POLR_DICT_ITEMS;
	const uint64_t n_blocks = (n_rows + per_block - 1) / per_block;
	lo->n_blocks = (uint32_t)(n_blocks ? n_blocks : 1);
	uint64_t at = 0;
	const auto take = [&at](uint64_t bytes) {
		const uint64_t off = at;
		at += (bytes + 15) & ~(uint64_t)15;
		return off;
	};
	lo->rep = take(capacity * 16); // (capacity is a multiple of 1024: the table's arrays need no rounding)
	lo->hash = take(capacity * 8);
	lo->state = take(capacity * 4);
	lo->first_row = take(capacity * 4);
	lo->code = take(capacity * 4);
	lo->slot_of_row = take(n_rows * 4);
	lo->row_of_code = take(n_rows * 4);
	lo->block_sums = take((uint64_t)lo->n_blocks * 4);
	lo->scalars = take(64);
	lo->n_long = lo->scalars + 32;
	lo->total = at;
}

// The scratch of the sort of n_codes >= 2 values: two arrays of sort records (ping and pong), a copy of every value's
// cell, its rank.  The tile sort leaves runs of POLR_DICT_SORT_TILE records; merge pass p doubles runs of
// POLR_DICT_SORT_TILE << p, until one run holds everything.
struct PolrDictSortLayout {
	uint64_t ping, pong, rep_old, rank, total;
	uint32_t n_tiles, n_merge_passes;
};
static inline void polr_dict_sort_layout(uint64_t n_codes, PolrDictSortLayout *lo) {
	lo->ping = 0;
	lo->pong = n_codes * POLR_DICT_REC_BYTES;
	lo->rep_old = 2 * n_codes * POLR_DICT_REC_BYTES;
	lo->rank = lo->rep_old + n_codes * 16;
	lo->total = lo->rank + n_codes * 4;
	lo->n_tiles = (uint32_t)((n_codes + POLR_DICT_SORT_TILE - 1) / POLR_DICT_SORT_TILE);
	lo->n_merge_passes = 0;
	for (uint64_t run = POLR_DICT_SORT_TILE; run < n_codes; run <<= 1) {
		lo->n_merge_passes++;
	}
}

// what an encoded column adds to the table's device bytes: the code column as polr_ht_export reports it, its validity
// array (POLR_DICT_NULL_INVALID over a column that has one), the representative cells
static inline uint64_t polr_dict_device_bytes(uint64_t n_rows, bool has_valid, uint32_t n_codes) {
	return polr_build_buffer_bytes(n_rows * 4) + (has_valid ? polr_build_buffer_bytes(n_rows) : 0) + (uint64_t)n_codes * 16;
}

#undef POLR_DP_REFUSE
