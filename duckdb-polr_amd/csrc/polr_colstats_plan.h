// duckdb-polr_amd/csrc/polr_colstats_plan.h -- a column-statistics request checked and laid out, as plain host code.
// No HIP in here: polr_colstats.hip describes the table or the pipeline, and allocates and launches what the plan says; a
// stand-alone host program drives the header alone (tests/colstats/colstats_plan_main.cpp).
//
// The plan:
//   * every refusal of polr_ht_column_stats and polr_pipeline_column_stats (include/polr_hip.h), in this order, each with its
//     message:
//       1. NULL handle, cols or stats                   POLR_E_INVALID
//       2. n_cols == 0                                  POLR_E_INVALID
//       3. more than POLR_MAX_STATS_COLS columns        POLR_E_UNSUPPORTED
//       4. table: a finalized table                     POLR_E_INVALID
//          pipeline: unknown flag bits                  POLR_E_INVALID
//       5. a cols[] entry beyond the columns            POLR_E_INVALID   (the first one, in order)
//   * the columns of a table: cols[] numbers them as a polr_ht_filter program does (polr_htfilter_col): keys first, then
//     payload; the columns of a pipeline are its probe columns;
//   * the launch shape of one column (polr_colstats_shape): a lane keeps POLR_COLSTATS_LOADS loads of 16 bytes in flight --
//     16 / width cells each, one cell where the rows come through a selection list --, a workgroup of 256 lanes covers a tile
//     of 256 x POLR_COLSTATS_LOADS loads, and at most POLR_COLSTATS_GRID_CAP workgroups (256 CUs x 8) are launched over all
//     columns of a call: a workgroup takes the tiles  blockIdx.x, blockIdx.x + grid, ...  of its column.  The rows in front
//     of the first 16-byte boundary of the cells and behind the last whole load are read one by one;
//   * one launch for all columns (polr_colstats_plan): grid = {the widest tile count among the columns, capped; n_cols};
//   * the partials scratch, one allocation: a record of POLR_COLSTATS_WORDS 8-byte words per workgroup, column after column
//     ([n_cols][grid]), then the combined record of every column ([n_cols]) -- what the second, small launch writes and
//     the host reads back;
//   * polr_colstats_finish(): a combined record as the caller sees it (min / max out of the order the kernel compares in);
//   * polr_colstats_finalize(): what polr_ht_finalize_auto_stats does -- which of "a statistics pass" and "perfect first" /
//     "hash table" follows from n_keys, the key flags, key_stats, n_valid and min / max.  Whether a perfect table is tried is
//     polr_build_auto_tries_perfect (polr_build_plan.h: the one definition), never restated here.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include "../../include/polr_hip.h"
#include "polr_build_plan.h"    // polr_build_buffer_bytes, polr_build_auto_tries_perfect
#include "polr_htfilter_plan.h" // polr_htfilter_col

#define POLR_COLSTATS_BLOCK 256u      // lanes of a workgroup
#define POLR_COLSTATS_LOADS 4u        // independent loads a lane keeps in flight
#define POLR_COLSTATS_VEC_BYTES 16u   // bytes of one load
#define POLR_COLSTATS_GRID_CAP 2048u  // workgroups of one launch, over all its columns
#define POLR_COLSTATS_WORDS 5u        // 8-byte words of a partial record: min, max (in compare order), n_valid, n_long, long_bytes
#define POLR_COLSTATS_SIGN (1ull << 63) // compare order: the extended value with its sign bit flipped if the column is signed, as uint64

struct PolrColStatsColumn { // a column as it stands
	uint32_t width, flags;  // flags: POLR_COL_SIGNED
	uint64_t data_addr;     // device address of its cells (only its low four bits matter: the scalar head)
};
struct PolrColStatsRequest {
	const char *who;        // "polr_ht_column_stats" / "polr_pipeline_column_stats"
	bool has_handle, has_cols, has_stats;
	bool is_table;
	bool finalized;         // table: kind != KIND_NONE
	uint32_t n_keys;        // table: columns below n_keys are keys
	uint32_t n_columns;     // table: n_keys + n_payload; pipeline: n_probe_cols
	uint32_t flags;         // pipeline: POLR_STATS_*
	bool selected;          // pipeline: a selection is in force AND POLR_STATS_SELECTED was given
	uint64_t n_rows;        // rows looked at: the table's, the pipeline's, or the selection's
	const uint32_t *cols;
	uint32_t n_cols;
};
struct PolrColStatsShape { // one column of n_rows rows
	uint32_t cells_per_load; // 16 / width; 1 through a selection list
	uint32_t tile_rows;      // rows of a workgroup tile: 256 x POLR_COLSTATS_LOADS loads
	uint64_t head_rows;      // rows in front of the first whole load (read one by one)
	uint64_t n_loads;        // whole loads behind the head
	uint64_t tail_rows;      // rows behind the last whole load
	uint64_t n_tiles;        // tiles the loads make
	uint32_t grid;           // workgroups this column alone would get: min(n_tiles, cap), at least 1 if there is a row
	uint64_t stride_rows;    // rows the grid covers before a workgroup takes its second tile: grid x tile_rows
};
struct PolrColStatsPlan {
	char err[256];
	uint32_t n_cols;
	PolrColStatsShape shape[POLR_MAX_STATS_COLS];
	uint32_t is_key[POLR_MAX_STATS_COLS], idx[POLR_MAX_STATS_COLS]; // table: which column of its kind
	uint32_t grid_x;                                              // 0: nothing is launched (no rows)
	uint64_t partials_off, result_off, record_bytes, scratch_bytes; // the scratch (scratch_bytes 0: none)
};

#define POLR_CS_REFUSE(code_, ...)                                                                                     \
	do {                                                                                                               \
		snprintf(pl.err, sizeof(pl.err), __VA_ARGS__);                                                                 \
		return (code_);                                                                                                \
	} while (0)

static inline bool polr_colstats_width_ok(uint32_t w) {
	return w == 1 || w == 2 || w == 4 || w == 8 || w == 16;
}

// the shape of one column; cap: the workgroups it may have
static inline void polr_colstats_shape(uint64_t n_rows, uint32_t width, uint64_t data_addr, bool selected, uint32_t cap,
                                       PolrColStatsShape &s) {
	s.cells_per_load = selected ? 1u : POLR_COLSTATS_VEC_BYTES / width;
	s.tile_rows = POLR_COLSTATS_BLOCK * POLR_COLSTATS_LOADS * s.cells_per_load;
	// a column's base is only as aligned as its cells: the rows up to the next 16-byte boundary are the head
	uint64_t head = 0;
	if (s.cells_per_load > 1) {
		const uint64_t off = data_addr & (POLR_COLSTATS_VEC_BYTES - 1);
		head = off ? (POLR_COLSTATS_VEC_BYTES - off + width - 1) / width : 0;
	}
	s.head_rows = head < n_rows ? head : n_rows;
	s.n_loads = (n_rows - s.head_rows) / s.cells_per_load;
	s.tail_rows = n_rows - s.head_rows - s.n_loads * s.cells_per_load;
	const uint64_t loads_per_tile = (uint64_t)POLR_COLSTATS_BLOCK * POLR_COLSTATS_LOADS;
	s.n_tiles = (s.n_loads + loads_per_tile - 1) / loads_per_tile;
	const uint64_t want = s.n_tiles ? s.n_tiles : (n_rows ? 1 : 0);
	s.grid = (uint32_t)(want < cap ? want : cap);
	s.stride_rows = (uint64_t)s.grid * s.tile_rows;
}

// shapes[n_columns]: every column of the table (keys first, then payload) or of the pipeline; not read before the request
// has passed refusals 1 to 4 -> POLR_OK, or POLR_E_* with pl.err set
static inline int polr_colstats_plan(const PolrColStatsRequest &rq, const PolrColStatsColumn *shapes, PolrColStatsPlan &pl) {
	pl.err[0] = 0;
	pl.n_cols = pl.grid_x = 0;
	pl.partials_off = pl.result_off = pl.scratch_bytes = 0;
	pl.record_bytes = POLR_COLSTATS_WORDS * 8ull;
	if (!rq.has_handle) {
		POLR_CS_REFUSE(POLR_E_INVALID, "%s: the %s is NULL", rq.who, rq.is_table ? "table" : "pipeline");
	}
	if (!rq.has_cols || !rq.cols) {
		POLR_CS_REFUSE(POLR_E_INVALID, "%s: cols is NULL", rq.who);
	}
	if (!rq.has_stats) {
		POLR_CS_REFUSE(POLR_E_INVALID, "%s: stats is NULL", rq.who);
	}
	if (rq.n_cols == 0) {
		POLR_CS_REFUSE(POLR_E_INVALID, "%s: no columns (n_cols is 0)", rq.who);
	}
	if (rq.n_cols > POLR_MAX_STATS_COLS) {
		POLR_CS_REFUSE(POLR_E_UNSUPPORTED, "%s: %u columns (at most %d in one call)", rq.who, rq.n_cols, POLR_MAX_STATS_COLS);
	}
	if (rq.is_table && rq.finalized) {
		POLR_CS_REFUSE(POLR_E_INVALID, "%s: the table is finalized (statistics are taken before polr_ht_finalize_*)", rq.who);
	}
	if (!rq.is_table && (rq.flags & ~POLR_STATS_SELECTED)) {
		POLR_CS_REFUSE(POLR_E_INVALID, "%s: flags 0x%x (0 or POLR_STATS_SELECTED)", rq.who, rq.flags);
	}
	for (uint32_t i = 0; i < rq.n_cols; i++) {
		if (rq.cols[i] >= rq.n_columns) {
			POLR_CS_REFUSE(POLR_E_INVALID, "%s: cols[%u]: column %u out of range (%u columns)", rq.who, i, rq.cols[i], rq.n_columns);
		}
	}
	pl.n_cols = rq.n_cols;
	const uint32_t cap = POLR_COLSTATS_GRID_CAP / rq.n_cols; // (at least 128)
	for (uint32_t i = 0; i < rq.n_cols; i++) {
		const PolrColStatsColumn &c = shapes[rq.cols[i]];
		if (!polr_colstats_width_ok(c.width)) {
			POLR_CS_REFUSE(POLR_E_UNSUPPORTED, "%s: cols[%u]: column %u of %u bytes", rq.who, i, rq.cols[i], c.width);
		}
		pl.is_key[i] = rq.is_table && polr_htfilter_col(rq.cols[i], rq.n_keys, pl.idx[i]) ? 1u : 0u;
		if (!rq.is_table) {
			pl.idx[i] = rq.cols[i];
		}
		polr_colstats_shape(rq.n_rows, c.width, c.data_addr, rq.selected, cap, pl.shape[i]);
		if (pl.shape[i].grid > pl.grid_x) {
			pl.grid_x = pl.shape[i].grid;
		}
	}
	if (pl.grid_x) {
		pl.partials_off = 0;
		pl.result_off = (uint64_t)rq.n_cols * pl.grid_x * pl.record_bytes;
		pl.scratch_bytes = polr_build_buffer_bytes(pl.result_off + (uint64_t)rq.n_cols * pl.record_bytes);
	}
	return POLR_OK;
}

// a combined record (or, for a column of no rows, nothing) as the caller sees it
static inline void polr_colstats_finish(const uint64_t *rec, uint64_t n_rows, uint32_t width, uint32_t flags, polr_col_stats &st) {
	st = polr_col_stats();
	st.n_rows = n_rows;
	st.width = width;
	st.flags = flags & POLR_COL_SIGNED;
	if (!rec || !rec[2]) {
		return; // no non-NULL row: min_value = max_value = 0
	}
	const uint64_t bias = (flags & POLR_COL_SIGNED) ? POLR_COLSTATS_SIGN : 0;
	st.min_value = (int64_t)(rec[0] ^ bias);
	st.max_value = (int64_t)(rec[1] ^ bias);
	st.n_valid = rec[2];
	st.n_long = rec[3];
	st.long_bytes = rec[4];
}

// ---- polr_ht_finalize_auto_stats -------------------------------------------------------------------------------------
enum PolrColStatsFinalize {
	POLR_CSF_AUTO = 0, // polr_ht_finalize_auto(ht, min, max): a perfect table is tried first, a duplicate falls back
	POLR_CSF_HASH = 1, // polr_ht_finalize_hash
};
// does the call run a statistics pass over key column 0?  Several keys or a flagged key take a hash table whatever the
// statistics say: the pass runs only for a caller who asked for key_stats.  (A finalized table is refused by the finalizer
// itself, before any pass.)
static inline bool polr_colstats_finalize_needs_pass(uint32_t n_keys, const uint32_t *key_flags, bool wants_stats) {
	return wants_stats || (n_keys == 1 && key_flags[0] == 0);
}
// ... and what follows from its numbers; *tries_perfect: whether polr_ht_finalize_auto will try a perfect table with them
// (had_pass false: st is not read)
static inline PolrColStatsFinalize polr_colstats_finalize(uint32_t n_keys, const uint32_t *key_flags, uint64_t n_rows_in,
                                                          bool had_pass, const polr_col_stats &st, bool *tries_perfect) {
	*tries_perfect = false;
	if (n_keys != 1 || key_flags[0] || !had_pass || st.n_valid == 0) {
		return POLR_CSF_HASH;
	}
	*tries_perfect = polr_build_auto_tries_perfect(n_keys, key_flags, n_rows_in, st.min_value, st.max_value,
	                                               (st.flags & POLR_COL_SIGNED) != 0);
	return POLR_CSF_AUTO;
}
