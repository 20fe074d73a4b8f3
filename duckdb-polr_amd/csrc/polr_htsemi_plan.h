// duckdb-polr_amd/csrc/polr_htsemi_plan.h -- a polr_ht_semi_filter request checked and laid out, as plain host code.
// No HIP in here: polr_htsemi.hip describes the table and the `by` tables, and allocates and launches what the plan says; a
// stand-alone host program drives the header alone (tests/htsemi/htsemi_plan_main.cpp).
//
// The plan:
//   * every refusal of the contract (include/polr_hip.h), in this order, each with its message:
//       1. NULL table                                   POLR_E_INVALID
//       2. a finalized table                            POLR_E_INVALID
//       3. a dictionary-encoded column                  POLR_E_INVALID   ("filter first, then encode")
//       4. more than POLR_MAX_SEMI_FILTERS filters      POLR_E_UNSUPPORTED  (then: filters NULL with n_filters > 0)
//       5. per filter, in order: NULL `by`; `by` not finalized; `by` the table itself; `by` on another device or context;
//          unknown flag bits; n_cols != by's key count (all POLR_E_INVALID); and per key, in order: a cols[] entry beyond the
//          table's columns (POLR_E_INVALID); a 16-byte column (POLR_E_UNSUPPORTED); the pairing rule of a join's keys
//          (pipe_key_pairing, polr_pipeline_plan.h: the one definition)
//   * the columns: cols[] numbers the table's columns as a polr_ht_filter program does (polr_htfilter_col);
//   * per filter and key column what the counting kernel computes with -- ONE arithmetic for the plain and the packed form
//     of `by`'s key: key |= (value - min) << shift, a value with value - min > range cannot match, a NULL is the code
//     range + 1 where NULL = NULL and otherwise cannot match.  Plain form: min 0, range all ones, shift 0 / 32, the value
//     sign-extended only for the signed key of a perfect table (what a join's fetch_key does); packed form: `by`'s KeyPack
//     and the signedness of the table's OWN column (a comparison by value), as fetch_key_packed;
//   * order[]: the filters as the device pass applies them, smallest device_bytes first (the cheapest index first, as LIP
//     orders its joins), ties by index.  The order changes the work, never the survivors;
//   * the scratch of the two passes: that of polr_ht_filter (polr_htfilter_plan);
//   * polr_htsemi_layout(): the table's one allocation afterwards.  A table never filtered before: exactly
//     polr_htfilter_layout.  A table filtered before carries its row list through the compaction as one more 4-byte column:
//     polr_htfilter_layout over the columns and that one -- carried_off is where the composed list (uploaded row numbers)
//     lands, and the list the compaction writes itself (row numbers of the table as it stood) lies at rows_off, unused.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/polr_hip.h"
#include "polr_htfilter_plan.h"
#include "polr_pipeline_plan.h" // KIND_*, pipe_key_pairing

struct PolrHtSemiBy { // the `by` table of one filter as it stands (nothing but has_by is read for a NULL one)
	bool has_by;
	bool finalized;   // kind != KIND_NONE
	bool is_ht;       // it is the table to be filtered
	bool same_place;  // same context, same device
	uint32_t kind;
	uint32_t n_keys;
	uint32_t key_width[POLR_NKEYS], key_flags[POLR_NKEYS]; // (flags: POLR_KEY_*)
	uint32_t key_signed; // of key 0 (a perfect table compares signed)
	KeyPack pack;
	uint64_t device_bytes;
};
struct PolrHtSemiRequest {
	bool has_ht;
	bool finalized;
	bool filtered; // polr_ht_filter or polr_ht_semi_filter succeeded on it before: the row list is carried
	bool has_dict;
	uint32_t dict_col;
	uint32_t n_keys, n_payload;
	uint64_t n_rows; // rows as the table holds them now
	const polr_semi_filter *filters;
	uint32_t n_filters;
	const PolrHtSemiBy *by; // [n_filters]
};
struct PolrHtSemiKey { // one key column of one filter, as the counting kernel computes with it
	uint32_t col;      // the table's column (numbering above)
	uint32_t width, sx;
	uint32_t shift, null_eq;
	int64_t min;
	uint64_t range;
};
struct PolrHtSemiFilter {
	uint32_t n_keys, anti;
	PolrHtSemiKey key[POLR_NKEYS];
};
struct PolrHtSemiPlan {
	char err[256];
	PolrHtSemiFilter f[POLR_MAX_SEMI_FILTERS]; // by the caller's index
	uint32_t order[POLR_MAX_SEMI_FILTERS];     // the device pass: order[i] is the caller's index of its i-th test
	uint32_t n_filters;
	bool carried;
	PolrHtFilterPlan scratch; // n_tiles, n_words, *_off, scratch_bytes
};
struct PolrHtSemiLayout {
	PolrHtFilterLayout lo; // data_off / valid_off [n_cols (+ 1: the carried list)], rows_off, desc_off, table_bytes
	uint32_t n_desc;       // descriptors the compaction reads: n_cols (+ 1)
	uint64_t list_off;     // the table's row list afterwards: rows_off, or the carried column's cells
};

// cols[n_keys + n_payload]: the keys, then the payload -> POLR_OK, or POLR_E_* with pl.err set
static inline int polr_htsemi_plan(const PolrHtSemiRequest &rq, const PolrHtFilterColumn *cols, PolrHtSemiPlan &pl) {
	pl.err[0] = 0;
	pl.n_filters = 0;
	pl.carried = false;
	if (!rq.has_ht) {
		POLR_HF_REFUSE(POLR_E_INVALID, "polr_ht_semi_filter: the table is NULL");
	}
	if (rq.finalized) {
		POLR_HF_REFUSE(POLR_E_INVALID,
		               "polr_ht_semi_filter: the table is finalized (a build side is filtered before polr_ht_finalize_*)");
	}
	if (rq.has_dict) {
		POLR_HF_REFUSE(POLR_E_INVALID, "polr_ht_semi_filter: payload column %u is dictionary-encoded: filter first, then encode",
		               rq.dict_col);
	}
	if (rq.n_filters > POLR_MAX_SEMI_FILTERS) {
		POLR_HF_REFUSE(POLR_E_UNSUPPORTED, "polr_ht_semi_filter: %u filters (at most %d in one call)", rq.n_filters,
		               POLR_MAX_SEMI_FILTERS);
	}
	if (rq.n_filters && (!rq.filters || !rq.by)) {
		POLR_HF_REFUSE(POLR_E_INVALID, "polr_ht_semi_filter: filters is NULL");
	}
	const uint32_t n_cols = rq.n_keys + rq.n_payload;
	for (uint32_t i = 0; i < rq.n_filters; i++) {
		const polr_semi_filter &sf = rq.filters[i];
		const PolrHtSemiBy &by = rq.by[i];
		if (!by.has_by) {
			POLR_HF_REFUSE(POLR_E_INVALID, "polr_ht_semi_filter: filter %u: `by` is NULL", i);
		}
		if (!by.finalized) {
			POLR_HF_REFUSE(POLR_E_INVALID, "polr_ht_semi_filter: filter %u: `by` is not finalized (its index is what is probed)", i);
		}
		if (by.is_ht) {
			POLR_HF_REFUSE(POLR_E_INVALID, "polr_ht_semi_filter: filter %u: `by` is the table itself", i);
		}
		if (!by.same_place) {
			POLR_HF_REFUSE(POLR_E_INVALID, "polr_ht_semi_filter: filter %u: `by` lives on another device or context", i);
		}
		if (sf.flags & ~POLR_SEMI_ANTI) {
			POLR_HF_REFUSE(POLR_E_INVALID, "polr_ht_semi_filter: filter %u: flags 0x%x (0 or POLR_SEMI_ANTI)", i, sf.flags);
		}
		if (sf.n_cols != by.n_keys || by.n_keys < 1 || by.n_keys > POLR_NKEYS) {
			POLR_HF_REFUSE(POLR_E_INVALID, "polr_ht_semi_filter: filter %u: %u columns for a %u-key table", i, sf.n_cols, by.n_keys);
		}
		PolrHtSemiFilter &f = pl.f[i];
		f.n_keys = by.n_keys;
		f.anti = (sf.flags & POLR_SEMI_ANTI) ? 1u : 0u;
		for (uint32_t c = 0; c < by.n_keys; c++) {
			const uint32_t col = sf.cols[c];
			if (col >= n_cols) {
				POLR_HF_REFUSE(POLR_E_INVALID, "polr_ht_semi_filter: filter %u key %u: column %u out of range", i, c, col);
			}
			const uint32_t width = cols[col].width;
			if (width == 16) {
				POLR_HF_REFUSE(POLR_E_UNSUPPORTED,
				               "polr_ht_semi_filter: filter %u key %u: column %u holds 16-byte cells (strings and wide composites "
				               "are not verified here)",
				               i, c, col);
			}
			const int pairing = pipe_key_pairing(width, by.key_width[c], by.key_flags[c]);
			if (pairing == PIPE_KEYS_WIDTHS_DIFFER) {
				POLR_HF_REFUSE(POLR_E_INVALID,
				               "polr_ht_semi_filter: filter %u key %u: column %u is %u bytes, the key of `by` %u bytes (a CAST'ed "
				               "key: polr_ht_set_key_flags(..., POLR_KEY_BY_VALUE) before `by` is finalized)",
				               i, c, col, width, by.key_width[c]);
			}
			if (pairing == PIPE_KEYS_NO_INTEGER) {
				POLR_HF_REFUSE(POLR_E_UNSUPPORTED, "polr_ht_semi_filter: filter %u key %u: column %u of %u bytes", i, c, col, width);
			}
			PolrHtSemiKey &k = f.key[c];
			k.col = col;
			k.width = width;
			if (by.pack.packed) {
				k.sx = (cols[col].flags & POLR_COL_SIGNED) ? 1u : 0u;
				k.shift = by.pack.shift[c];
				k.null_eq = (by.pack.null_eq >> c) & 1u;
				k.min = by.pack.min[c];
				k.range = by.pack.range[c];
			} else {
				k.sx = (c == 0 && by.kind == KIND_PERFECT && by.key_signed) ? 1u : 0u;
				k.shift = 32u * c;
				k.null_eq = 0;
				k.min = 0;
				k.range = ~0ull;
			}
		}
	}
	pl.n_filters = rq.n_filters;
	for (uint32_t i = 0; i < rq.n_filters; i++) {
		pl.order[i] = i;
	}
	std::stable_sort(pl.order, pl.order + rq.n_filters,
	                 [&](uint32_t a, uint32_t b) { return rq.by[a].device_bytes < rq.by[b].device_bytes; });
	pl.carried = rq.filtered;
	// the scratch: polr_ht_filter's, for a program that keeps every row
	PolrHtFilterRequest hf = {};
	hf.has_ht = true;
	hf.n_keys = rq.n_keys;
	hf.n_payload = rq.n_payload;
	hf.n_rows = rq.n_rows;
	if (const int rc = polr_htfilter_plan(hf, cols, pl.scratch)) {
		POLR_HF_REFUSE(rc, "%s", pl.scratch.err);
	}
	return POLR_OK;
}

static inline void polr_htsemi_layout(const PolrHtFilterColumn *cols, uint32_t n_cols, bool carried, uint64_t n_kept,
                                      PolrHtSemiLayout &sl) {
	std::vector<PolrHtFilterColumn> all(cols, cols + n_cols);
	if (carried) {
		all.push_back(PolrHtFilterColumn{4, 0, 0, 1, 0});
	}
	sl.n_desc = (uint32_t)all.size();
	polr_htfilter_layout(all.data(), sl.n_desc, n_kept, sl.lo);
	sl.list_off = carried ? sl.lo.data_off[n_cols] : sl.lo.rows_off;
}
