// duckdb-polr_amd/csrc/polr_build_plan.h -- the rules of a build side, as plain host code: its limits, the shapes an upload
// takes, the range of a perfect table, when polr_ht_finalize_auto tries one, the capacity and kind of a hash table, the
// packed form of a composite key, the buffers a finalized table consists of, and what a metadata blob from another rank
// must say before anything is allocated from it.  Each rule stands here once, behind every route to a table:
// polr_ht_upload_columns / polr_ht_upload_rows and the finalizers, polr_pht_upload, polr_ht_export / polr_ht_alloc_like
// (polr_capi.hip), polr_ht_from_output (polr_fromout_plan.h), the dictionary and the hash aggregate (their capacity).
// No HIP in here: the entry points describe the request, call the plan, turn a refusal into the context's error
// (POLR_FAIL(ctx, code, "%s", plan.err)) and allocate and launch what the plan says; a stand-alone host program drives the
// header alone (tests/buildplan/build_plan_main.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/polr_hip.h"
#include "polr_pipeline_plan.h" // POLR_NKEYS, KIND_*

// ---- limits ------------------------------------------------------------------------------------------------------------
#define POLR_BUILD_MAX_ROWS 0xFFFFFFF0ull  // build row ids are 32-bit: a build side has fewer rows than this
#define POLR_BUILD_MAX_PAYLOAD 62u         // payload columns of a table that can be shipped (PolrHtMeta describes that many)
#define POLR_BUILD_MAX_SLOTS (1ull << 31)  // slots of a hash table (32-bit slot space), and values a perfect table spans
#define POLR_BUILD_MIN_SLOTS 1024ull       // ... and its floor
#define POLR_BUILD_MAX_RUN (1ull << 25)    // rows of one build key: the expansion counter's range
#define POLR_BUILD_SMALL_RANGE 1000000ull  // a perfect table of at most this range is tried however sparse it is
#define POLR_BUILD_META_MAGIC 0x504F4C52u

static inline bool polr_build_key_width_ok(uint32_t w) { // cells of a key column
	return w == 1 || w == 2 || w == 4 || w == 8;
}
static inline bool polr_build_cell_width_ok(uint32_t w) { // cells of a payload column: 16 is a string cell
	return polr_build_key_width_ok(w) || w == 16;
}
// bytes of a device buffer asked for with n bytes: what DevBuf::alloc makes (an empty buffer is 16 bytes), what
// polr_ht_export lists and polr_ht_alloc_like allocates -- never more, the receiving side copies that many
static inline uint64_t polr_build_buffer_bytes(uint64_t n) {
	return n ? n : 16;
}

// Composite keys that do not fit the plain {key0 | key1 << 32} form: column c contributes (value - min[c]) << shift[c],
// value sign- or zero-extended by the BUILD column's type; a probe value outside [min, min + range] cannot match.
// (The device structs of polr_device.h embed it; it travels inside PolrHtMeta.)
struct KeyPack {
	uint32_t packed; // 0: plain form
	uint32_t shift[POLR_NKEYS];
	uint32_t sx[POLR_NKEYS]; // sign-extend column c (the BUILD column; the probe side's: StageExt::key_sx)
	uint32_t null_eq;        // bit c: IS NOT DISTINCT FROM on column c -- NULL is the code range[c] + 1, on both sides
	uint32_t pad[2];
	int64_t min[POLR_NKEYS];
	uint64_t range[POLR_NKEYS];
};
static_assert(sizeof(KeyPack) == 112 && offsetof(KeyPack, min) == 48, "the kernels and the metadata blob read this layout");

struct PolrBuildPlan { // what every plan below starts with: the text of its refusal
	char err[256] = {};
};

#define POLR_BP_REFUSE(code_, ...)                                                                                     \
	do {                                                                                                               \
		snprintf(pl.err, sizeof(pl.err), __VA_ARGS__);                                                                 \
		return (code_);                                                                                                \
	} while (0)

// ---- upload shape ------------------------------------------------------------------------------------------------------
static inline int polr_build_check_rows(uint64_t n_rows, PolrBuildPlan &pl) {
	if (n_rows >= POLR_BUILD_MAX_ROWS) {
		POLR_BP_REFUSE(POLR_E_UNSUPPORTED, "build side of %llu rows exceeds the 32-bit row-id space", (unsigned long long)n_rows);
	}
	return POLR_OK;
}

static inline int polr_build_check_col_width(uint32_t width, PolrBuildPlan &pl) {
	if (!polr_build_cell_width_ok(width)) {
		POLR_BP_REFUSE(POLR_E_UNSUPPORTED, "column width %u not supported (1,2,4,8,16)", width);
	}
	return POLR_OK;
}

static inline int polr_build_check_keys(size_t n_keys, const uint32_t *key_width, PolrBuildPlan &pl) {
	if (n_keys < 1 || n_keys > POLR_MAX_KEYS) {
		POLR_BP_REFUSE(POLR_E_UNSUPPORTED, "%zu equality keys per join not supported (1..%d)", n_keys, POLR_MAX_KEYS);
	}
	for (size_t c = 0; c < n_keys; c++) {
		if (key_width[c] > 8) {
			POLR_BP_REFUSE(POLR_E_UNSUPPORTED, "VARCHAR join keys are outside this path");
		}
		if (!polr_build_key_width_ok(key_width[c])) {
			POLR_BP_REFUSE(POLR_E_UNSUPPORTED, "join key of %u bytes", key_width[c]);
		}
	}
	return POLR_OK;
}

// the row blob of polr_ht_upload_rows: n_cols cells at col_offset[] of col_width[] bytes, one validity bit per column (and
// one for the row) in the row's first bytes
static inline int polr_build_check_row_layout(uint32_t row_width, uint32_t n_cols, const uint32_t *col_offset,
                                              const uint32_t *col_width, PolrBuildPlan &pl) {
	for (uint32_t c = 0; c < n_cols; c++) {
		if (!polr_build_cell_width_ok(col_width[c]) || (uint64_t)col_offset[c] + col_width[c] > row_width) {
			POLR_BP_REFUSE(POLR_E_INVALID, "row layout: column %u (offset %u, width %u) does not fit row width %u", c, col_offset[c],
			               col_width[c], row_width);
		}
	}
	if (((uint64_t)n_cols + 1 + 7) / 8 > row_width) {
		POLR_BP_REFUSE(POLR_E_INVALID, "row layout: validity bytes exceed row width");
	}
	return POLR_OK;
}

// ---- perfect tables ----------------------------------------------------------------------------------------------------
struct PolrPerfectPlan : PolrBuildPlan {
	uint64_t range; // max - min
	uint64_t size;  // slots: range + 1
	uint64_t words; // 32-bit words of the bit table
};

static inline bool polr_build_stats_ordered(int64_t min_value, int64_t max_value, bool is_signed) {
	return is_signed ? max_value >= min_value : (uint64_t)max_value >= (uint64_t)min_value;
}

// [min_value, max_value] in the key's own order (the statistics come from outside the library: the difference is taken
// modulo 2^64, which are the bits the subtraction in the key's type has wherever that one is defined)
static inline int polr_build_perfect_range(int64_t min_value, int64_t max_value, bool is_signed, PolrPerfectPlan &pl) {
	pl.range = (uint64_t)max_value - (uint64_t)min_value;
	pl.size = pl.words = 0;
	if (!polr_build_stats_ordered(min_value, max_value, is_signed) || pl.range >= POLR_BUILD_MAX_SLOTS) {
		POLR_BP_REFUSE(POLR_E_INVALID, "perfect hash range [%lld, %lld] invalid", (long long)min_value, (long long)max_value);
	}
	pl.size = pl.range + 1;
	pl.words = (pl.size + 31) / 32;
	return POLR_OK;
}

// polr_pht_upload: a perfect table the caller built
static inline int polr_build_pht_upload(uint32_t key_width, int64_t min_value, int64_t max_value, bool is_signed,
                                        PolrPerfectPlan &pl) {
	if (polr_build_perfect_range(min_value, max_value, is_signed, pl) || !polr_build_key_width_ok(key_width)) {
		POLR_BP_REFUSE(POLR_E_INVALID, "perfect table shape invalid");
	}
	return POLR_OK;
}

// polr_ht_finalize_auto: is a perfect table tried first?  One plain key, ordered statistics, at least one row, and keys
// that are dense (range / POLR_DENSE_FACTOR <= rows) or -- like the reference's planner, plan_comparison_join.cpp:118,125 --
// of a range of at most 1 M values (a 125 KB bit table, however few of its bits are set: a filtered dimension)
static inline bool polr_build_auto_tries_perfect(uint32_t n_keys, const uint32_t *key_flags, uint64_t n_rows_in, int64_t min_value,
                                                 int64_t max_value, bool is_signed) {
	if (n_keys != 1 || key_flags[0] || n_rows_in == 0) {
		return false;
	}
	PolrPerfectPlan pl;
	if (polr_build_perfect_range(min_value, max_value, is_signed, pl)) {
		return false;
	}
	return pl.range / POLR_DENSE_FACTOR <= n_rows_in || pl.range <= POLR_BUILD_SMALL_RANGE;
}

// ---- hash tables -------------------------------------------------------------------------------------------------------
// composite keys outside the plain {key0 | key1 << 32} form are packed exactly (KeyPack)
static inline bool polr_build_needs_key_pack(uint32_t n_keys, const uint32_t *key_width, const uint32_t *key_flags) {
	if (n_keys >= 3) {
		return true;
	}
	for (uint32_t c = 0; c < n_keys; c++) {
		if (key_flags[c]) {
			return true; // compared by value (a CAST on one side) or NULL = NULL: the packed form does both exactly
		}
	}
	return n_keys == 2 && (key_width[0] > 4 || key_width[1] > 4);
}

static inline uint32_t polr_build_null_eq_mask(uint32_t n_keys, const uint32_t *key_flags) {
	uint32_t null_eq = 0;
	for (uint32_t c = 0; c < n_keys; c++) {
		null_eq |= (key_flags[c] & POLR_KEY_NULL_EQUAL) ? (1u << c) : 0u;
	}
	return null_eq;
}

struct PolrCapacityPlan : PolrBuildPlan {
	uint64_t capacity;
};

// slots of an open-addressing table of n entries: load factor <= 0.5 like PointerTableCapacity (join_hashtable.hpp:265-267),
// floor 1024 slots, a power of two
static inline int polr_build_capacity(uint64_t n, PolrCapacityPlan &pl) {
	pl.capacity = POLR_BUILD_MIN_SLOTS;
	while (pl.capacity / 2 < n && pl.capacity < (1ull << 63)) { // (capacity < 2 n, without the product)
		pl.capacity <<= 1;
	}
	if (pl.capacity > POLR_BUILD_MAX_SLOTS) {
		POLR_BP_REFUSE(POLR_E_UNSUPPORTED, "hash table of %llu slots exceeds the 32-bit slot space", (unsigned long long)pl.capacity);
	}
	return POLR_OK;
}

struct PolrKindPlan : PolrBuildPlan {
	uint64_t max_run;
	uint32_t kind; // KIND_S8 or KIND_S16
};

// longest_run, sentinel_count: what the build kernel counted (the rows of the sentinel key are a run of their own).
// KIND_S8, {key32, row} slots: unique 32-bit keys in plain form
static inline int polr_build_hash_kind(uint64_t longest_run, uint64_t sentinel_count, uint32_t n_keys, uint32_t key0_width,
                                       bool packed, PolrKindPlan &pl) {
	pl.max_run = longest_run > sentinel_count ? longest_run : sentinel_count;
	pl.kind = KIND_NONE;
	if (pl.max_run >= POLR_BUILD_MAX_RUN) {
		POLR_BP_REFUSE(POLR_E_UNSUPPORTED, "a build key repeats more than 2^25 times: outside the expansion counter range");
	}
	pl.kind = pl.max_run <= 1 && n_keys == 1 && key0_width == 4 && !packed ? KIND_S8 : KIND_S16;
	return POLR_OK;
}

struct PolrKeyPackPlan : PolrBuildPlan {
	KeyPack pack;
};

// mm[2 c], mm[2 c + 1]: min and max of key column c over the rows that count (min > max: there is none); col_flags[c]:
// POLR_COL_SIGNED of the build column.  Column c takes the bits of its range -- one code more where NULL = NULL -- above
// those of the columns before it.
static inline int polr_build_key_pack(uint32_t n_keys, const long long *mm, uint32_t null_eq, const uint32_t *col_flags,
                                      PolrKeyPackPlan &pl) {
	pl.pack = KeyPack();
	pl.pack.packed = 1;
	pl.pack.null_eq = null_eq;
	uint32_t shift = 0;
	for (uint32_t c = 0; c < n_keys; c++) {
		const bool empty = mm[2 * c] > mm[2 * c + 1]; // no row with valid keys at all
		const int64_t lo = empty ? 0 : mm[2 * c], hi = empty ? 0 : mm[2 * c + 1];
		const uint64_t range = (uint64_t)hi - (uint64_t)lo;
		// (a NULL = NULL column has one more code, range + 1: NULL)
		const bool null_eq_col = ((null_eq >> c) & 1u) != 0;
		const uint64_t top = range + (null_eq_col ? 1u : 0u);
		uint32_t bits = 0;
		while (bits < 64 && (top >> bits) != 0) {
			bits++;
		}
		if (shift + bits > 64 || (null_eq_col && top == 0)) {
			POLR_BP_REFUSE(POLR_E_UNSUPPORTED,
			               "composite key of %u columns needs more than 64 bits (column %u: range %llu after %u bits)", n_keys, c,
			               (unsigned long long)range, shift);
		}
		pl.pack.shift[c] = shift;
		pl.pack.sx[c] = (col_flags[c] & POLR_COL_SIGNED) ? 1u : 0u;
		pl.pack.min[c] = lo;
		pl.pack.range[c] = range;
		shift += bits;
	}
	return POLR_OK;
}

// ---- a finalized table: its description, its buffers -------------------------------------------------------------------
// What polr_ht_export writes and polr_ht_alloc_like reads: plain integers and the key pack.
struct PolrHtMeta {
	uint32_t magic, kind, n_keys, n_payload, key_signed, is_dense, has_null, sentinel_start, sentinel_count, pad;
	uint64_t n_rows_in, n_rows, capacity, max_run, range;
	int64_t min_value, max_value;
	uint32_t key_width[POLR_MAX_KEYS];
	uint32_t key_flags[POLR_MAX_KEYS];
	uint32_t key_sem[POLR_MAX_KEYS]; // POLR_KEY_* (polr_ht_set_key_flags)
	KeyPack pack;
	uint32_t payload_width[POLR_BUILD_MAX_PAYLOAD];
	uint32_t payload_flags[POLR_BUILD_MAX_PAYLOAD];
	uint8_t payload_has_valid[POLR_BUILD_MAX_PAYLOAD];
};
static_assert(sizeof(PolrHtMeta) == 816 && offsetof(PolrHtMeta, capacity) == 56 && offsetof(PolrHtMeta, payload_width) == 256,
              "ranks exchange this layout");

enum { POLR_BUF_TABLE = 0, POLR_BUF_ROWIDS = 1, POLR_BUF_COL_DATA = 2, POLR_BUF_COL_VALID = 3 };
struct PolrBuildBuffer {
	uint32_t what; // POLR_BUF_*
	uint32_t col;  // POLR_BUF_COL_*: the payload column
	uint64_t bytes;
};

// The buffers of a finalized table in the order polr_ht_export lists them: the bits of a perfect table or the slots of a
// hash table, the row ids of a KIND_S16 table, then per payload column its cells and, if it has one, its validity array.
// A perfect table's columns have a cell per slot, a hash table's one per build row.
static inline void polr_build_buffers(uint32_t kind, uint64_t capacity, uint64_t n_rows_in, uint32_t n_payload,
                                      const uint32_t *payload_width, const uint8_t *payload_has_valid,
                                      std::vector<PolrBuildBuffer> &out) {
	out.clear();
	const uint64_t rows = kind == KIND_PERFECT ? capacity : n_rows_in;
	const uint64_t table = kind == KIND_PERFECT ? (capacity + 31) / 32 * 4 : capacity * (kind == KIND_S8 ? 8 : 16);
	out.push_back(PolrBuildBuffer {POLR_BUF_TABLE, 0, polr_build_buffer_bytes(table)});
	if (kind == KIND_S16) {
		out.push_back(PolrBuildBuffer {POLR_BUF_ROWIDS, 0, polr_build_buffer_bytes(n_rows_in * 4)});
	}
	for (uint32_t i = 0; i < n_payload; i++) {
		out.push_back(PolrBuildBuffer {POLR_BUF_COL_DATA, i, polr_build_buffer_bytes(rows * payload_width[i])});
		if (payload_has_valid[i]) {
			out.push_back(PolrBuildBuffer {POLR_BUF_COL_VALID, i, polr_build_buffer_bytes(rows)});
		}
	}
}

// a metadata blob before anything is allocated from it: the kernels read with these widths, capacities and ranges
static inline int polr_build_check_meta(const PolrHtMeta &m, PolrBuildPlan &pl) {
	if (m.magic != POLR_BUILD_META_MAGIC || m.n_payload > POLR_BUILD_MAX_PAYLOAD || m.n_keys < 1 || m.n_keys > POLR_MAX_KEYS) {
		POLR_BP_REFUSE(POLR_E_INVALID, "bad table metadata");
	}
	if (m.kind != KIND_PERFECT && m.kind != KIND_S8 && m.kind != KIND_S16) {
		POLR_BP_REFUSE(POLR_E_INVALID, "bad table kind in metadata");
	}
	for (uint32_t i = 0; i < m.n_keys; i++) {
		if (!polr_build_key_width_ok(m.key_width[i])) {
			POLR_BP_REFUSE(POLR_E_INVALID, "bad table metadata: key %u of %u bytes", i, m.key_width[i]);
		}
	}
	for (uint32_t i = 0; i < m.n_payload; i++) {
		if (!polr_build_cell_width_ok(m.payload_width[i])) {
			POLR_BP_REFUSE(POLR_E_INVALID, "bad table metadata: payload column %u of %u bytes", i, m.payload_width[i]);
		}
	}
	if (m.kind == KIND_PERFECT) {
		if (m.range >= POLR_BUILD_MAX_SLOTS || m.capacity != m.range + 1) {
			POLR_BP_REFUSE(POLR_E_INVALID, "bad table metadata: a perfect table of %llu slots over a range of %llu",
			               (unsigned long long)m.capacity, (unsigned long long)m.range);
		}
	} else if (m.capacity < POLR_BUILD_MIN_SLOTS || m.capacity > POLR_BUILD_MAX_SLOTS || (m.capacity & (m.capacity - 1))) {
		POLR_BP_REFUSE(POLR_E_INVALID, "bad table metadata: a hash table of %llu slots", (unsigned long long)m.capacity);
	}
	if (m.n_rows_in >= POLR_BUILD_MAX_ROWS) {
		POLR_BP_REFUSE(POLR_E_INVALID, "bad table metadata: %llu build rows", (unsigned long long)m.n_rows_in);
	}
	return POLR_OK;
}
