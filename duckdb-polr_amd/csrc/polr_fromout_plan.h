// duckdb-polr_amd/csrc/polr_fromout_plan.h -- a polr_ht_from_output request checked and laid out, as plain host code.
// No HIP in here: polr_fromout.hip resolves the column references against the pipeline (polr_out_col), hands their shapes
// and the output's counts over and allocates and launches what the plan says; a stand-alone host program drives the header
// alone (tests/fromout/fromout_plan_main.cpp).
//
// The plan:
//   * every refusal of the contract (include/polr_hip.h) with its message -- polr_fromout_check() those that need no column
//     shape (it runs before the references are resolved), polr_fromout_plan() all of them;
//   * fixed[]: the columns of 1, 2, 4 and 8 bytes, keys and payload alike, ordered by the slot of the output's row ids
//     that indexes their source (stable, so equal slots keep the request's order): a workgroup of the gather kernel loads
//     the row ids of one slot and serves the whole run of that slot's columns with them; n_slots: the distinct slots, i.e.
//     the row ids read per output row; group_first[g] .. group_first[g + 1]: the run of fixed[] that slot group g is (the
//     kernel's grid is chunks x groups);
//   * strings[]: the VARCHAR payload columns, each with the guard it needs (a source the library uploaded whose heap never
//     came);
//   * the table's memory: ONE allocation that holds every column's cells and validity array (a table of 66 columns would
//     otherwise make 132; on the five-column workload of tools/bench_from_output.py one instead of ten took the call from
//     1.31 to 1.22 ms), each at an offset that is a multiple of 256 bytes, and behind them the gather kernel's descriptor
//     array, a few KB that the table keeps; the string heaps are allocations of their own, their sizes are measured on
//     the device; and the scratch of the string passes, one allocation as well.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/polr_hip.h"
#include "polr_build_plan.h" // the limits and cell widths of every build side

#define POLR_FROMOUT_MAX_PAYLOAD POLR_BUILD_MAX_PAYLOAD // what polr_ht_export carries
#define POLR_FROMOUT_MAX_ROWS POLR_BUILD_MAX_ROWS       // the bound of polr_ht_upload_columns: build row ids are 32-bit
#define POLR_FROMOUT_MAX_SLOTS 9u            // 1 + POLR_MAX_JOINS: the probe row and a build row per join

struct PolrFromoutColumn { // a column reference as polr_out_col resolved it
	uint32_t resolved;     // 0: polr_out_col refused the reference
	uint32_t slot;         // the output's row ids that index the source: 0 probe, 1 + j join j
	uint32_t width, flags; // of the source column (flags: POLR_COL_SIGNED)
	uint32_t has_valid;    // the source has a validity array
	uint32_t owned;        // the library uploaded the source (not a caller's POLR_COL_DEVICE memory)
	uint32_t rebased;      // VARCHAR: its cells point into a device heap (polr_*_set_*_heaps)
};
struct PolrFromoutRequest {
	bool has_out, has_result, has_keys, has_payload; // the pointers of the call that are not NULL
	bool fused;                                      // the output has a fused GROUP BY sink
	uint32_t n_keys, n_payload;
	uint64_t n_rows, n_chunks; // of the output (polr_out_stats); polr_fromout_check does not read them
};
struct PolrFromoutFixed {
	uint32_t col; // 0 .. n_keys - 1: key column; n_keys + i: payload column i
	uint32_t slot, width;
};
struct PolrFromoutString {
	uint32_t col;             // as above (always a payload column)
	uint32_t slot;
	uint32_t needs_heap_guard; // a long non-NULL cell among the output rows is POLR_E_INVALID: the heap never came
};
struct PolrFromoutDesc { // one fixed-width column as the gather kernel reads it (device addresses)
	const uint8_t *src_data, *src_valid; // src_valid NULL: every source row is valid
	uint8_t *dst_data, *dst_valid;
	uint32_t width, slot;
};
struct PolrFromoutPlan {
	char err[200];
	std::vector<PolrFromoutFixed> fixed;
	std::vector<PolrFromoutString> strings;
	uint32_t n_slots;                 // distinct slots among fixed[]
	uint32_t group_first[POLR_FROMOUT_MAX_SLOTS + 1]; // [n_slots + 1]: fixed[group_first[g] .. group_first[g + 1]) share a slot
	std::vector<uint64_t> data_off, valid_off; // [n_keys + n_payload]: where the column's cells (n_rows * width bytes) and
	                                           // its validity array (n_rows bytes) begin in the table's allocation
	uint64_t desc_off;                // ... and the descriptor array, fixed.size() records of PolrFromoutDesc
	uint64_t table_bytes;             // that allocation (never empty: DevBuf::alloc would make 16 bytes of nothing)
	// scratch of the string passes, 8-byte words, one allocation in this order:
	uint64_t row_off_words;           // n_rows per VARCHAR column,
	uint64_t chunk_words;             // 2 * n_chunks per VARCHAR column (byte totals and their prefix, polr_strout.hip),
	uint64_t tail_words;              // 2 per VARCHAR column: the heap bytes and the long cells, read back together
};

#define POLR_FO_REFUSE(code_, ...)                                                                                     \
	do {                                                                                                               \
		snprintf(pl.err, sizeof(pl.err), __VA_ARGS__);                                                                 \
		return (code_);                                                                                                \
	} while (0)

#define POLR_FROMOUT_ALIGN 256ull // of every array inside the table's allocation

#define polr_fromout_alloc_bytes polr_build_buffer_bytes // DevBuf::alloc

// what can be refused before a column reference is looked at -> POLR_OK, or POLR_E_* with pl.err set
static inline int polr_fromout_check(const PolrFromoutRequest &rq, PolrFromoutPlan &pl) {
	pl.err[0] = 0;
	if (!rq.has_out || !rq.has_result || !rq.has_keys) {
		POLR_FO_REFUSE(POLR_E_INVALID, "polr_ht_from_output: %s is NULL", !rq.has_out ? "the output" : !rq.has_result ? "out" : "keys");
	}
	if (!rq.has_payload && rq.n_payload) {
		POLR_FO_REFUSE(POLR_E_INVALID, "%u payload columns at NULL", rq.n_payload);
	}
	if (rq.fused) {
		POLR_FO_REFUSE(POLR_E_INVALID, "the output has a fused GROUP BY sink: it holds group cells, no row ids to materialise");
	}
	if (rq.n_keys < 1 || rq.n_keys > POLR_MAX_KEYS) {
		POLR_FO_REFUSE(POLR_E_UNSUPPORTED, "%u equality keys per join not supported (1..%d)", rq.n_keys, POLR_MAX_KEYS);
	}
	if (rq.n_payload > POLR_FROMOUT_MAX_PAYLOAD) {
		POLR_FO_REFUSE(POLR_E_UNSUPPORTED, "%u payload columns (at most %u)", rq.n_payload, POLR_FROMOUT_MAX_PAYLOAD);
	}
	return POLR_OK;
}

static inline void polr_fromout_clear(PolrFromoutPlan &pl) {
	pl.fixed.clear();
	pl.strings.clear();
	pl.data_off.clear();
	pl.valid_off.clear();
	pl.n_slots = 0;
	pl.table_bytes = pl.desc_off = pl.row_off_words = pl.chunk_words = pl.tail_words = 0;
}

// The layout alone, for n_cols columns whose widths are cell widths (1, 2, 4, 8, 16) and fewer than 2^32 rows: fixed[] by
// slot and the slot groups, strings[], every column's place in the one allocation, the descriptors behind them, the scratch
// of the string passes.  Shared by polr_fromout_plan() below and by polr_pipeline_from_output (polr_pipesrc_plan.h), whose
// columns are all of one kind.
static inline int polr_fromout_layout(uint64_t n_rows, uint64_t n_chunks, const PolrFromoutColumn *cols, uint32_t n_cols,
                                      PolrFromoutPlan &pl) {
	pl.data_off.resize(n_cols);
	pl.valid_off.resize(n_cols);
	uint64_t at = 0; // (at most 66 columns of fewer than 2^32 rows and 17 bytes a row: far from 2^64)
	for (uint32_t c = 0; c < n_cols; c++) {
		pl.data_off[c] = at;
		at += (n_rows * cols[c].width + POLR_FROMOUT_ALIGN - 1) / POLR_FROMOUT_ALIGN * POLR_FROMOUT_ALIGN;
		pl.valid_off[c] = at;
		at += (n_rows + POLR_FROMOUT_ALIGN - 1) / POLR_FROMOUT_ALIGN * POLR_FROMOUT_ALIGN;
		if (cols[c].width == 16) {
			pl.strings.push_back(PolrFromoutString{c, cols[c].slot, cols[c].owned && !cols[c].rebased ? 1u : 0u});
		} else {
			pl.fixed.push_back(PolrFromoutFixed{c, cols[c].slot, cols[c].width});
		}
	}
	std::stable_sort(pl.fixed.begin(), pl.fixed.end(),
	                 [](const PolrFromoutFixed &a, const PolrFromoutFixed &b) { return a.slot < b.slot; });
	for (size_t i = 0; i < pl.fixed.size(); i++) {
		if (i == 0 || pl.fixed[i].slot != pl.fixed[i - 1].slot) {
			if (pl.n_slots == POLR_FROMOUT_MAX_SLOTS) {
				POLR_FO_REFUSE(POLR_E_INVALID, "columns from more than %u slots of row ids", POLR_FROMOUT_MAX_SLOTS);
			}
			pl.group_first[pl.n_slots++] = (uint32_t)i;
		}
	}
	pl.group_first[pl.n_slots] = (uint32_t)pl.fixed.size();
	pl.desc_off = at;
	pl.table_bytes = polr_fromout_alloc_bytes(at + pl.fixed.size() * sizeof(PolrFromoutDesc));
	pl.row_off_words = (uint64_t)pl.strings.size() * n_rows;
	pl.chunk_words = (uint64_t)pl.strings.size() * 2ull * n_chunks;
	pl.tail_words = (uint64_t)pl.strings.size() * 2ull;
	return POLR_OK;
}

// cols[n_keys + n_payload]: the keys, then the payload -> POLR_OK, or POLR_E_* with pl.err set
static inline int polr_fromout_plan(const PolrFromoutRequest &rq, const PolrFromoutColumn *cols, PolrFromoutPlan &pl) {
	polr_fromout_clear(pl);
	const int rc = polr_fromout_check(rq, pl);
	if (rc) {
		return rc;
	}
	const uint32_t n_cols = rq.n_keys + rq.n_payload;
	for (uint32_t c = 0; c < n_cols; c++) {
		const bool is_key = c < rq.n_keys;
		const char *what = is_key ? "key" : "payload column";
		const uint32_t idx = is_key ? c : c - rq.n_keys;
		if (!cols[c].resolved) {
			POLR_FO_REFUSE(POLR_E_INVALID, "%s %u: no such column in the output's pipeline", what, idx);
		}
		const uint32_t w = cols[c].width;
		if (is_key && w > 8) {
			POLR_FO_REFUSE(POLR_E_UNSUPPORTED, "key %u: VARCHAR join keys are outside this path", idx);
		}
		if (is_key ? !polr_build_key_width_ok(w) : !polr_build_cell_width_ok(w)) {
			POLR_FO_REFUSE(POLR_E_UNSUPPORTED, "%s %u: cells of %u bytes", what, idx, w);
		}
	}
	if (rq.n_rows >= POLR_FROMOUT_MAX_ROWS) {
		POLR_FO_REFUSE(POLR_E_UNSUPPORTED, "build side of %llu rows exceeds the 32-bit row-id space", (unsigned long long)rq.n_rows);
	}
	return polr_fromout_layout(rq.n_rows, rq.n_chunks, cols, n_cols, pl);
}
