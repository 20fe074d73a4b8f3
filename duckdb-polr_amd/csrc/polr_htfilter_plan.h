// duckdb-polr_amd/csrc/polr_htfilter_plan.h -- a polr_ht_filter request checked and laid out, as plain host code.
// No HIP in here: polr_htfilter.hip describes the table, hands the program over and allocates and launches what the plan
// says; a stand-alone host program drives the header alone (tests/htfilter/htfilter_plan_main.cpp).
//
// The plan:
//   * the column numbering of a filter program over a build side: as polr_ht_upload_rows numbers them, keys first, then
//     payload -- col < n_keys is key column col, otherwise payload column col - n_keys (polr_htfilter_col);
//   * every refusal of the contract (include/polr_hip.h) that needs no device, in this order, each with its message:
//       1. NULL table                                   POLR_E_INVALID
//       2. a finalized table                            POLR_E_INVALID
//       3. a dictionary-encoded column                  POLR_E_INVALID   ("filter first, then encode")
//       4. a table filtered already                     POLR_E_INVALID   (once per table)
//       5. what polr_filter_plan() refuses, `col` beyond the table's columns included, with its code and its message
//          behind "filter expression: "
//     (the heap guard is the one refusal that needs the device: it comes after all of these);
//   * guard[]: the VARCHAR columns some CMP / IN / LIKE leaf reads that the library uploaded and whose heap never came: a
//     non-NULL cell longer than 12 bytes in one of them is POLR_E_INVALID, decided by a pass over the length words;
//   * the scratch of the two passes: one pass bit per table row in 64-row words, whole tiles of POLR_HTFILTER_TILE rows
//     (the words behind the table's last row are written as 0), a 32-bit count and a 64-bit first output row per tile, the
//     total;
//   * polr_htfilter_layout(), once the kept count is known: the table's memory afterwards, ONE allocation -- per column
//     its cells and, if the column had a validity array, its validity array, each at a multiple of 256 bytes; then the
//     row list (the uploaded row number of every kept row, 4 bytes each); then the copy descriptors, one per column.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/polr_hip.h"
#include "polr_build_plan.h" // polr_build_buffer_bytes
#include "polr_filter_plan.h"

#define POLR_HTFILTER_TILE 1024u      // rows of a tile: one count, one first output row
#define POLR_HTFILTER_TILE_WORDS 16u  // ... in 64-row pass-bit words
#define POLR_HTFILTER_ALIGN 256ull    // of every array inside the table's allocation
#define POLR_HTFILTER_NO_ARRAY (~0ull) // valid_off of a column without a validity array

struct PolrHtFilterColumn { // a column of the table as it stands
	uint32_t width, flags; // flags: POLR_COL_SIGNED
	uint32_t has_valid;    // it has a validity array
	uint32_t owned;        // the library uploaded it (not a caller's POLR_COL_DEVICE memory)
	uint32_t rebased;      // VARCHAR: its cells point into a device heap
};
struct PolrHtFilterRequest {
	bool has_ht;
	bool finalized;          // kind != KIND_NONE
	bool filtered;           // polr_ht_filter succeeded on it before
	bool has_dict;           // some payload column is dictionary-encoded ...
	uint32_t dict_col;       // ... this one (the first)
	uint32_t n_keys, n_payload;
	uint64_t n_rows;         // rows as uploaded
	const polr_filter_node *nodes;
	uint32_t n_nodes;
	const polr_filter_value *values;
	uint32_t n_values;
};
struct PolrHtFilterDesc { // one column as the compaction kernel reads it (device addresses)
	const uint8_t *src_data, *src_valid; // src_valid NULL: every row is valid, and dst_valid is NULL too
	uint8_t *dst_data, *dst_valid;
	uint32_t width, pad;
};
struct PolrHtFilterPlan {
	char err[256];
	PolrFilterPlan fx;            // the lowered program (fx.cols[].col: table columns in the numbering above)
	std::vector<uint32_t> guard;  // table columns that need the heap guard, in the order of fx.cols[]
	uint64_t n_tiles, n_words;    // tiles of the table; pass-bit words (whole tiles)
	// the scratch, one allocation, byte offsets: words, first output rows and the total (8 bytes each), counts (4 bytes each)
	uint64_t bits_off, base_off, total_off, count_off, scratch_bytes;
};
struct PolrHtFilterLayout {
	std::vector<uint64_t> data_off, valid_off; // [n_keys + n_payload]; valid_off: POLR_HTFILTER_NO_ARRAY without an array
	uint64_t rows_off, desc_off;
	uint64_t table_bytes; // the allocation (never empty: DevBuf::alloc makes 16 bytes of nothing)
};

#define POLR_HF_REFUSE(code_, ...)                                                                                     \
	do {                                                                                                               \
		snprintf(pl.err, sizeof(pl.err), __VA_ARGS__);                                                                 \
		return (code_);                                                                                                \
	} while (0)

// table column `col` of a filter program: is it a key, and which one of its kind
static inline bool polr_htfilter_col(uint32_t col, uint32_t n_keys, uint32_t &idx) {
	const bool is_key = col < n_keys;
	idx = is_key ? col : col - n_keys;
	return is_key;
}

static inline uint64_t polr_htfilter_up(uint64_t n) {
	return (n + POLR_HTFILTER_ALIGN - 1) / POLR_HTFILTER_ALIGN * POLR_HTFILTER_ALIGN;
}

// cols[n_keys + n_payload]: the keys, then the payload (not read for a NULL, finalized, encoded or filtered table)
// -> POLR_OK, or POLR_E_* with pl.err set
static inline int polr_htfilter_plan(const PolrHtFilterRequest &rq, const PolrHtFilterColumn *cols, PolrHtFilterPlan &pl) {
	pl.err[0] = 0;
	pl.guard.clear();
	pl.n_tiles = pl.n_words = pl.bits_off = pl.base_off = pl.total_off = pl.count_off = pl.scratch_bytes = 0;
	if (!rq.has_ht) {
		POLR_HF_REFUSE(POLR_E_INVALID, "polr_ht_filter: the table is NULL");
	}
	if (rq.finalized) {
		POLR_HF_REFUSE(POLR_E_INVALID, "polr_ht_filter: the table is finalized (a build side is filtered before polr_ht_finalize_*)");
	}
	if (rq.has_dict) {
		POLR_HF_REFUSE(POLR_E_INVALID, "polr_ht_filter: payload column %u is dictionary-encoded: filter first, then encode", rq.dict_col);
	}
	if (rq.filtered) {
		POLR_HF_REFUSE(POLR_E_INVALID, "polr_ht_filter: the table was filtered already (once per table)");
	}
	const uint32_t n_cols = rq.n_keys + rq.n_payload;
	std::vector<PolrFilterColumn> shapes(n_cols ? n_cols : 1);
	for (uint32_t c = 0; c < n_cols; c++) {
		shapes[c].width = cols[c].width;
		shapes[c].is_signed = cols[c].flags & POLR_COL_SIGNED;
	}
	if (const int rc = polr_filter_plan(rq.nodes, rq.n_nodes, rq.values, rq.n_values, shapes.data(), n_cols, pl.fx)) {
		POLR_HF_REFUSE(rc, "filter expression: %s", pl.fx.err);
	}
	for (uint32_t g = 0; g < pl.fx.n_cols; g++) {
		const PolrHtFilterColumn &c = cols[pl.fx.cols[g].col];
		if (pl.fx.cols[g].needs_cell && c.width == 16 && c.owned && !c.rebased) {
			pl.guard.push_back(pl.fx.cols[g].col);
		}
	}
	pl.n_tiles = (rq.n_rows + POLR_HTFILTER_TILE - 1) / POLR_HTFILTER_TILE;
	pl.n_words = pl.n_tiles * POLR_HTFILTER_TILE_WORDS;
	pl.bits_off = 0;
	pl.base_off = pl.bits_off + pl.n_words * 8;
	pl.total_off = pl.base_off + pl.n_tiles * 8;
	pl.count_off = pl.total_off + 8;
	pl.scratch_bytes = polr_build_buffer_bytes(pl.count_off + pl.n_tiles * 4);
	return POLR_OK;
}

// the table's one allocation, given the kept count (at most 66 columns of fewer than 2^32 rows and 17 bytes a row: far from
// 2^64)
static inline void polr_htfilter_layout(const PolrHtFilterColumn *cols, uint32_t n_cols, uint64_t n_kept, PolrHtFilterLayout &lo) {
	lo.data_off.assign(n_cols, 0);
	lo.valid_off.assign(n_cols, POLR_HTFILTER_NO_ARRAY);
	uint64_t at = 0;
	for (uint32_t c = 0; c < n_cols; c++) {
		lo.data_off[c] = at;
		at += polr_htfilter_up(n_kept * cols[c].width);
		if (cols[c].has_valid) {
			lo.valid_off[c] = at;
			at += polr_htfilter_up(n_kept);
		}
	}
	lo.rows_off = at;
	at += polr_htfilter_up(n_kept * 4);
	lo.desc_off = at;
	lo.table_bytes = polr_build_buffer_bytes(at + (uint64_t)n_cols * sizeof(PolrHtFilterDesc));
}
