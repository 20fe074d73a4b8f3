// duckdb-polr_amd/csrc/polr_device.h -- device-side data layout of the POLAR path (gfx950).
//
// Everything the path kernels touch lives in HBM in these shapes:
//   probe side   : SoA columns exactly as the host hands them over (FLAT vectors), optional
//                  selection list of the tuples that enter the multiplexer.
//   build side   : SoA key/payload columns indexed by build row + ONE index over the key:
//       KIND_PERFECT : bit map over [min, max] (1 bit per key value, L2 resident: <= 125 KB) and
//                      payload columns re-ordered by (key - min), as the reference's perfect table.
//       KIND_S8      : open addressing, 8-byte slots {key32, row}; unique 32-bit keys (FK -> PK).
//       KIND_S16     : open addressing, 16-byte slots {key64, start, count}; `rowids[start..+count)`
//                      holds the rows of that key contiguously (bucket-contiguous runs instead of
//                      the reference's pointer chains).
//     load factor <= 0.5, linear probing, so a lookup touches one 64-byte line in the common case.
//   intermediates: never in HBM.  Tuples between joins live in per-wave LDS queues as row-id
//                  tuples (late materialisation); only final tuples are written, as row ids.
#pragma once

#include <stdint.h>

#include "polr_pipeline_plan.h" // POLR_KMAX, POLR_PMAX, POLR_NKEYS, POLR_NPREDS, KIND_*: shared with the host's plan
#include "polr_build_plan.h"    // KeyPack: shared with the host's build-side plan
#include "polr_fuseagg_plan.h"  // POLR_FUSEAGG_*: the cell layout of the fused ungrouped sink, shared with its host plan

// Device code names the address space of what it loads from: a pointer rebuilt from an integer (descriptors travel as
// 64-bit words through LDS and scalar registers) is a GENERIC pointer to the compiler, and a generic access is a FLAT
// instruction -- it counts against the LDS counter (lgkmcnt) as well as the memory counter, so every wait for an LDS
// read would also wait for all key-column loads in flight.  as_global()/as_lds() give GLOBAL_/DS_ instructions.
#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
#define POLR_GLOBAL __attribute__((address_space(1)))
#define POLR_LDS __attribute__((address_space(3)))
#define POLR_CONST __attribute__((address_space(4))) // constant memory: a wave-uniform address is read through the scalar cache
template <class T>
__device__ __forceinline__ POLR_GLOBAL T *as_global(T *p) {
	return (POLR_GLOBAL T *)p;
}
template <class T>
__device__ __forceinline__ POLR_LDS T *as_lds(T *p) {
	return (POLR_LDS T *)p;
}
// one 16-byte load from global memory (the HIP vector classes do not bind to address-space qualified references)
typedef uint32_t polr_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 load_global_x4(const POLR_GLOBAL uint32_t *p) {
	const polr_u32x4 v = *(const POLR_GLOBAL polr_u32x4 *)p;
	return make_uint4(v.x, v.y, v.z, v.w);
}
#endif

#define POLR_WMAX (1 + POLR_KMAX)
// per-round counters are sharded by workgroup so a table-sized round does not serialise thousands of
// atomics on k words; readers sum the shards
#define POLR_NSHARD 32 // (the router sums the shards with one half-wave per counter: keep it 32)

#define S8_EMPTY_ROW 0xFFFFFFFFu
#define S16_EMPTY_KEY 0xFFFFFFFFFFFFFFFFull

struct DevCol {
	const uint8_t *data;
	const uint8_t *valid; // nullptr = all valid
	uint32_t width;
	uint32_t flags; // bit0 signed
};

struct DevJoin {
	uint32_t kind;
	uint32_t n_keys;
	uint32_t key_width[POLR_NKEYS];
	uint32_t key_signed;
	int32_t key_src_join[POLR_NKEYS];
	int32_t key_src_col[POLR_NKEYS];
	uint32_t n_payload;
	uint64_t mask;         // hash: capacity - 1
	int64_t min_value;     // perfect
	uint64_t range;        // perfect: max - min
	const void *table;     // S8: uint2[capacity]; S16: uint4[capacity]; perfect: uint32 bit words
	const uint32_t *rowids; // S16: runs of build rows; perfect: nullptr
	uint32_t sentinel_start; // S16 side entry for key == S16_EMPTY_KEY
	uint32_t sentinel_count;
	const DevCol *payload; // n_payload columns, indexed by build id (perfect: by key - min)
	uint32_t n_preds;      // non-equality conditions (polr_join_desc)
	uint32_t pred_op[POLR_NPREDS];
	int32_t pred_src_join[POLR_NPREDS];
	int32_t pred_src_col[POLR_NPREDS];
	uint32_t pred_build_col[POLR_NPREDS];
};

struct DevPath {
	uint32_t order[POLR_KMAX];
};

// One join of one join order, fully resolved on the host at pipeline creation so the path kernel
// needs no pointer chasing: which tuple slot indexes the key column(s), where the key column lives,
// which index to probe and which tuple slot receives the matched build row.
// The uncommon parts of a stage -- composite keys beyond the plain two-column form, non-equality conditions -- live in
// an extension record in global memory (StageDesc::ext): the descriptor every probe wave keeps in LDS stays small (the
// per-wave LDS of the generic kernel is K descriptors + the queues, and it is staged again whenever the join order of a
// unit differs from the last one's).
// two string_t cells (16 bytes: length, then 12 inline characters or a 4-byte prefix + a pointer; string_type.hpp:23-28)
// hold the same string -- the verifying condition of a VARCHAR join key (POLR_CMP_STR_EQ): the key itself is the 64-bit
// hash the engine computed for the bucket, as in JoinHashTable::Hash + RowOperations::Match
#define POLR_PRED_STR_EQ 8u
// (cells in registers: the one definition of "the same string" -- the join condition below and the VARCHAR group columns of
// the general GROUP BY sink, polr_agg.hip.  Lengths first, then the characters: the padding of an inline cell and the
// pointer of a long one are never compared.)
__device__ __forceinline__ bool polr_str_equal(const uint4 &a, const uint4 &b) {
	if (a.x != b.x) {
		return false;
	}
	if (a.x <= 12u) {
		// (inline: compare the characters, not the padding)
		const uint32_t n = a.x;
		const uint32_t wa[3] = {a.y, a.z, a.w}, wb[3] = {b.y, b.z, b.w};
		bool same = true;
#pragma unroll
		for (uint32_t i = 0; i < 3; i++) {
			const uint32_t left = n > 4u * i ? n - 4u * i : 0u; // characters of this word that belong to the string
			const uint32_t mask = left >= 4u ? 0xFFFFFFFFu : (left ? (1u << (8u * left)) - 1u : 0u);
			same = same && ((wa[i] ^ wb[i]) & mask) == 0u;
		}
		return same;
	}
	if (a.y != b.y) { // (the prefix)
		return false;
	}
	const uint8_t *pa = (const uint8_t *)(((uint64_t)a.w << 32) | a.z), *pb = (const uint8_t *)(((uint64_t)b.w << 32) | b.z);
	for (uint32_t i = 4; i < a.x; i++) {
		if (pa[i] != pb[i]) {
			return false;
		}
	}
	return true;
}
__device__ __forceinline__ bool polr_str_cells_equal(const uint8_t *a_cell, const uint8_t *b_cell) {
	return polr_str_equal(*(const uint4 *)a_cell, *(const uint4 *)b_cell);
}

struct StageExt {
	// every key column of the join, in packed form (KeyPack)
	uint32_t key_width[POLR_NKEYS]; // of the column the PROBE side reads (a CAST'ed key: not the build column's)
	uint32_t key_sx[POLR_NKEYS];    // ... and whether it is sign-extended
	int32_t key_slot[POLR_NKEYS];
	const uint8_t *key_data[POLR_NKEYS];
	const uint8_t *key_valid[POLR_NKEYS];
	KeyPack pack;
	// non-equality conditions, evaluated on every (tuple, build row) pair the equalities produce: left = column
	// pred_data[c] at the row in tuple slot pred_slot[c], right = build column pred_bdata[c] at the build id
	uint32_t n_preds;
	uint32_t pred_op[POLR_NPREDS];
	uint32_t pred_width[POLR_NPREDS];
	uint32_t pred_sx[POLR_NPREDS];
	int32_t pred_slot[POLR_NPREDS];
	uint32_t pred_pad;
	const uint8_t *pred_data[POLR_NPREDS];
	const uint8_t *pred_valid[POLR_NPREDS];
	const uint8_t *pred_bdata[POLR_NPREDS];
	const uint8_t *pred_bvalid[POLR_NPREDS];
};

struct StageDesc {
	uint32_t kind;
	uint32_t n_keys;
	uint32_t key_width[2];
	uint32_t key_signed;
	int32_t key_slot[2];        // tuple slot whose value indexes key column c (0 = probe row)
	int32_t out_slot;           // tuple slot that receives this join's build id, -1: not carried
	const uint8_t *key_data[2]; // (plain form: one key, or two of <= 32 bits; packed composites: StageExt)
	const uint8_t *key_valid[2];
	const void *table;
	const uint32_t *rowids;
	uint64_t mask;
	int64_t min_value;
	uint64_t range;
	uint32_t sentinel_start;
	uint32_t sentinel_count;
	uint32_t unique;   // 1: at most one build row per key (perfect table or longest run == 1); 2: keys may repeat
	uint32_t lds_off1; // flat pipelines: 1 + dword offset of this join's bit table in the workgroup's LDS table area; 0 = HBM
	uint32_t packed;   // composite key in packed form: fetch it through ext
	uint32_t n_preds;  // non-equality conditions: evaluate them through ext
	const StageExt *ext; // nullptr unless packed or n_preds
};
#define STAGE_DESC_DWORDS (sizeof(StageDesc) / 4)

// One stage of one join order as the FLAT pool kernel keeps it in scalar registers: exactly the words of a FlatStage
// (polr_flat_device.h), written by the host when the pipeline is created (the descriptors are constant for the pipeline's
// life) so that a probe wave whose next unit belongs to another join order fetches the K records of that order with
// 16-byte-aligned loads issued back to back -- nothing to select, nothing to chase.  A record beyond the pipeline's last
// join (position >= k) is all zero: an inert stage.
struct FlatStageRec {
	const uint32_t *keys;
	const uint8_t *valid;
	const uint32_t *table;
	uint32_t kind_lds; // kind | lds_off1 << 8
	uint32_t a, b;     // perfect: min, range (32-bit modular); hash: slot mask, range (unused)
	uint32_t out_slot; // 1 + the join's index in the original order
	uint32_t pad[2];
};
#define FLAT_STAGE_WORDS 10u // the dwords of a record that a FlatStage holds
static_assert(sizeof(FlatStageRec) == 48 && sizeof(FlatStageRec) % 16 == 0, "three 16-byte granules per record");
static_assert(offsetof(FlatStageRec, kind_lds) == 24 && offsetof(FlatStageRec, pad) == 4 * FLAT_STAGE_WORDS, "FlatStageRec layout");

// the record of one resolved stage (host and device agree on it here, once)
inline FlatStageRec flat_stage_rec(const StageDesc &d, uint32_t join_index) {
	FlatStageRec r;
	r.keys = (const uint32_t *)d.key_data[0];
	r.valid = d.key_valid[0];
	r.table = (const uint32_t *)d.table;
	r.kind_lds = d.kind | (d.lds_off1 << 8);
	r.a = d.kind == KIND_PERFECT ? (uint32_t)d.min_value : (uint32_t)d.mask;
	r.b = (uint32_t)d.range;
	r.out_slot = 1u + join_index;
	r.pad[0] = r.pad[1] = 0;
	return r;
}

struct DevPipeline {
	uint32_t k;
	uint32_t n_paths;
	uint32_t n_probe_cols;
	uint32_t W;             // slots carried per tuple: 1 (probe row) + carried build ids
	uint32_t materialize;   // 1: all build ids carried, slot 1+j = join j
	uint32_t ext;           // some stage has an extension record (packed composite key, non-equality conditions): POLR_EXT kernels
	uint32_t mult;          // 1 (counting variant, pool launch): tuples carry a multiplicity in one more slot behind the W id slots
	                        // -- some join's matches are folded into it instead of being handed on one by one (polr_gen_device.h)
	int32_t slot_of_join[POLR_KMAX]; // slot index holding join j's build id, or -1
	const DevCol *probe_cols;
	const uint32_t *sel;    // nullptr = identity
	uint64_t n_tuples;
	DevJoin joins[POLR_KMAX];
	DevPath paths[POLR_PMAX];
	const StageDesc *stages; // [n_paths][POLR_KMAX], resolved per (join order, position)
	// flat pipelines (polr_flat_device.h): every join keyed by one 4-byte probe column with <= 1 build row per key
	uint32_t flat;            // 1: the counting variant may run on the flat pipeline
	uint32_t n_lds_tables;    // bit tables kept in LDS for the whole run
	uint32_t lds_table_dwords; // their total size
	uint32_t pad2;
	const uint32_t *lds_table_src[POLR_KMAX]; // HBM source of LDS table t
	uint32_t lds_table_off[POLR_KMAX];        // dword offset in the LDS table area
	uint32_t lds_table_len[POLR_KMAX];        // dwords
	const FlatStageRec *flat_stages;          // [n_paths][POLR_KMAX]: `stages` in the flat kernel's own form
};

// one routed slice; must match polr_round in include/polr_hip.h
struct DevRound {
	uint64_t begin;
	uint64_t count;
	uint32_t path;
	uint32_t emit;
};

// chunked output (a DataChunk stream of row ids)
struct FusedSink;
struct FusedAggSink;
struct DevOut {
	uint32_t *ids;          // [W_out][max_chunks * chunk_capacity]
	uint32_t *chunk_count;  // [max_chunks]
	uint32_t *cursor;       // [0] = next free chunk, [1] = overflow flag
	uint64_t slot_stride;   // max_chunks * chunk_capacity
	uint32_t chunk_capacity;
	uint32_t max_chunks;
	uint32_t W_out;
	uint32_t pad;
	const FusedSink *fused; // nullptr: row ids are written (see FusedSink below)
	const FusedAggSink *agg; // the generic pool kernel's ungrouped sink (FusedAggSink below); at most one of the two is set
};

// ---- aggregate sinks (polr_agg.hip; the flat pipeline's fused GROUP BY, polr_flat_device.h) ---------------------------
struct DevAgg {
	DevCol src;
	uint32_t slot; // 0: probe row ids, 1 + j: build row ids of join j
	uint32_t fn;
};

#define POLR_MAX_AGGS 8
struct DevAggSet {
	DevAgg a[POLR_MAX_AGGS];
	uint32_t n;
	uint32_t pad;
};

struct DevGroupKey {
	DevCol src;
	uint32_t slot;
	uint32_t n_values;
	int64_t min_value;
};

#define POLR_MAX_GROUP_KEYS 3
struct DevGroupSet {
	DevGroupKey k[POLR_MAX_GROUP_KEYS];
	uint32_t n;
	uint32_t n_groups;
};

// A perfect-hash GROUP BY of COUNT / SUM aggregates FUSED into the last join of an emitting flat pipeline
// (polr_out_fuse_grouped): instead of writing its row ids, a surviving tuple is folded into the group cells of its
// workgroup's table -- [n_tables][n_groups][1 + 2 n_aggs] 64-bit words (rows of the group; per aggregate sum, count) in
// global memory, updated with atomics nobody waits for; the tables are summed when the result is read.
#define POLR_DEV_AGG_COUNT_STAR 0u // (= POLR_AGG_COUNT_STAR / _COUNT / _SUM of polr_hip.h: static_assert in polr_agg.hip)
#define POLR_DEV_AGG_COUNT 1u
#define POLR_DEV_AGG_SUM 2u
#define POLR_DEV_AGG_MIN 3u // (the ungrouped sink of the generic kernel, FusedAggSink below, takes these two as well)
#define POLR_DEV_AGG_MAX 4u
struct FusedSink {
	DevGroupSet groups;
	DevAggSet aggs;
	unsigned long long *cells;
	unsigned long long *dropped;
	uint32_t n_tables, words_per_table;
};

// Ungrouped aggregates FUSED into the generic pool kernel (polr_out_fuse_aggregate): where a final tuple would leave as row
// ids (gen_out_write, polr_gen_device.h) its wave folds it into the cells of its workgroup's table instead --
// [n_tables][1 + 3 n_aggs] 64-bit words in global memory (layout, combining rule and reset values: polr_fuseagg_plan.h),
// updated with atomics nobody waits for; the tables are combined when the result is read.
static_assert(POLR_MAX_AGGS == POLR_FUSEAGG_MAX_AGGS, "aggregates per sink");
struct FusedAggSink {
	DevAggSet aggs;
	unsigned long long *cells;
	uint32_t n_tables, words_per_table;
};

__host__ __device__ inline uint64_t polr_murmurhash64(uint64_t x) {
	// same finaliser as the reference (src/include/duckdb/common/types/hash.hpp:22-29); the device
	// table is re-bucketed so any hash would do, keeping this one keeps bucket statistics comparable
	x ^= x >> 32;
	x *= 0xd6e8feb86659fd93ULL;
	x ^= x >> 32;
	x *= 0xd6e8feb86659fd93ULL;
	x ^= x >> 32;
	return x;
}

#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
// 64-bit hash of a string_t cell's value: the length, then the characters 8 at a time (the last group zero-padded) --
// inline strings from the cell (padding masked off), long ones through the pointer, never past the string's end.  Equal
// strings hash equally whatever their padding or heap address; a NULL row's cell must not be handed in.
__device__ __forceinline__ uint64_t polr_str_hash(const uint4 &c) {
	const uint32_t n = c.x;
	uint64_t h = polr_murmurhash64(0x9E3779B97F4A7C15ull ^ n);
	if (n <= 12u) {
		uint32_t w[3] = {c.y, c.z, c.w};
#pragma unroll
		for (uint32_t i = 0; i < 3; i++) {
			const uint32_t left = n > 4u * i ? n - 4u * i : 0u;
			w[i] &= left >= 4u ? 0xFFFFFFFFu : (left ? (1u << (8u * left)) - 1u : 0u);
		}
		if (n) {
			h = polr_murmurhash64(h ^ (((uint64_t)w[1] << 32) | w[0]));
		}
		if (n > 8u) {
			h = polr_murmurhash64(h ^ w[2]);
		}
		return h;
	}
	const uint8_t *p = (const uint8_t *)(((uint64_t)c.w << 32) | c.z);
	uint32_t i = 0;
	for (; i + 8u <= n; i += 8u) {
		uint64_t w;
		__builtin_memcpy(&w, p + i, 8);
		h = polr_murmurhash64(h ^ w);
	}
	if (i < n) {
		uint64_t w = 0;
		for (uint32_t j = 0; i + j < n; j++) {
			w |= (uint64_t)p[i + j] << (8u * j);
		}
		h = polr_murmurhash64(h ^ w);
	}
	return h;
}
#endif

// ---- the rules every device kernel shares ----------------------------------------------------------------------------
// Data formats and key semantics that build, scan, probe and sink kernels must agree on bit for bit -- one definition
// each.  They read through POLR_GLOBAL pointers (kernels that hold generic ones convert at the call with as_global).
#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
// ---- wave helpers
__device__ __forceinline__ uint32_t uni(uint32_t v) {
	return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
	uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
	uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
	return ((uint64_t)hi << 32) | lo;
}
template <class T>
__device__ __forceinline__ const T *uniptr(const T *p) {
	return (const T *)uni64((uint64_t)p);
}
// rank of this lane among the lanes of `mask` below it
__device__ __forceinline__ uint32_t lane_rank(uint64_t mask) {
	return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, uint32_t lane) {
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t o = __shfl_up(v, d, 64);
		if ((int)lane >= d) {
			v += o;
		}
	}
	return v;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) { // the same sum in every lane
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) {
		v += __shfl_xor(v, d, 64);
	}
	return v;
}

// ---- cells: a 1/2/4/8-byte value widened to 64 bits, sign- or zero-extended
__device__ __forceinline__ uint64_t load_cell(const POLR_GLOBAL uint8_t *p, uint32_t width, bool sign_extend) {
	switch (width) {
	case 1: {
		const uint8_t v = *p;
		return sign_extend ? (uint64_t)(int64_t)(int8_t)v : (uint64_t)v;
	}
	case 2: {
		const uint16_t v = *(const POLR_GLOBAL uint16_t *)p;
		return sign_extend ? (uint64_t)(int64_t)(int16_t)v : (uint64_t)v;
	}
	case 4: {
		const uint32_t v = *(const POLR_GLOBAL uint32_t *)p;
		return sign_extend ? (uint64_t)(int64_t)(int32_t)v : (uint64_t)v;
	}
	default:
		return *(const POLR_GLOBAL uint64_t *)p;
	}
}
// one cell of a column, as a signed 64-bit value (the column's flags say whether it is signed)
__device__ __forceinline__ long long load_col_cell(const DevCol &c, uint64_t row) {
	return (long long)load_cell(as_global(c.data) + row * c.width, c.width, (c.flags & 1u) != 0);
}

// ---- tuples of row ids: slot 0 the probe row, the others build ids
template <int W>
struct Tuple {
	uint32_t s[W];
};
template <int W>
__device__ __forceinline__ uint32_t tuple_slot(const Tuple<W> &t, int32_t slot) {
	uint32_t v = t.s[0];
#pragma unroll
	for (int q = 1; q < W; q++) {
		v = (q == slot) ? t.s[q] : v;
	}
	return v;
}

// composite key in packed form (KeyPack): per column (value - min) << shift; a value outside the build side's
// [min, min + range] cannot match.  Everything comes from the stage's extension record.  A function of its own (like
// preds_hold below): inlined into every place a stage fetches keys, the uncommon paths made the POLR_EXT objects the
// slowest of the build by minutes -- the pipelines that take them can afford a call.
template <int W>
__device__ __attribute__((noinline)) bool fetch_key_packed(const POLR_GLOBAL StageExt *d, uint32_t n_keys, const Tuple<W> &t,
                                                           uint64_t &key) {
	bool valid = true;
	key = 0;
	for (uint32_t c = 0; c < n_keys; c++) {
		const uint32_t row = tuple_slot<W>(t, d->key_slot[c]);
		const POLR_GLOBAL uint8_t *kv = as_global(d->key_valid[c]);
		const uint32_t w = d->key_width[c];
		// (by VALUE: the probe column's own width and signedness -- a CAST'ed key; a value outside the build side's range
		// cannot match, whichever type could or could not hold it)
		const uint64_t v = load_cell(as_global(d->key_data[c]) + (uint64_t)row * w, w, d->key_sx[c] != 0);
		uint64_t off = v - (uint64_t)d->pack.min[c];
		if (kv && !kv[row]) {
			if ((d->pack.null_eq >> c) & 1u) {
				off = d->pack.range[c] + 1u; // IS NOT DISTINCT FROM: NULL is a key value of its own
			} else {
				valid = false;
			}
		} else if (off > d->pack.range[c]) {
			valid = false;
		}
		key |= off << d->pack.shift[c];
	}
	if (!valid) {
		key = 0;
	}
	return valid;
}

// the join's non-equality conditions on one (tuple, build row) pair (RowOperations::Match, row_match.cpp:59-119:
// both sides valid and `left OP right`); descriptors come from the extension record -- joins that have any are rare
template <int W>
__device__ __attribute__((noinline)) bool preds_hold(const POLR_GLOBAL StageExt *d, uint32_t n_preds, const Tuple<W> &t,
                                                     uint32_t id) {
	bool ok = true;
	for (uint32_t c = 0; c < n_preds; c++) {
		const uint32_t row = tuple_slot<W>(t, d->pred_slot[c]);
		const uint32_t w = d->pred_width[c];
		const bool sx = d->pred_sx[c] != 0;
		const POLR_GLOBAL uint8_t *lv = as_global(d->pred_valid[c]);
		const POLR_GLOBAL uint8_t *rv = as_global(d->pred_bvalid[c]);
		if ((lv && !lv[row]) || (rv && !rv[id])) {
			ok = false;
		}
		if (d->pred_op[c] == POLR_PRED_STR_EQ) { // the strings behind a VARCHAR key's hash
			ok = ok && polr_str_cells_equal(d->pred_data[c] + (uint64_t)row * 16u, d->pred_bdata[c] + (uint64_t)id * 16u);
			continue;
		}
		const uint64_t l = load_cell(as_global(d->pred_data[c]) + (uint64_t)row * w, w, sx);
		const uint64_t r = load_cell(as_global(d->pred_bdata[c]) + (uint64_t)id * w, w, sx);
		bool h;
		if (w == 8 && !sx) {
			switch (d->pred_op[c]) {
			case 0: h = l == r; break; // (POLR_CMP_EQ: the verifying comparison behind a hashed composite key)
			case 1: h = l != r; break;
			case 2: h = l < r; break;
			case 3: h = l > r; break;
			case 4: h = l <= r; break;
			default: h = l >= r; break;
			}
		} else {
			const int64_t a = (int64_t)l, b = (int64_t)r; // (narrow unsigned values are zero-extended: same order)
			switch (d->pred_op[c]) {
			case 0: h = a == b; break;
			case 1: h = a != b; break;
			case 2: h = a < b; break;
			case 3: h = a > b; break;
			case 4: h = a <= b; break;
			default: h = a >= b; break;
			}
		}
		ok = ok && h;
	}
	return ok;
}

// ---- indexes (layouts: top of this file)
// KIND_PERFECT: is `key` inside [min, min + range] (compared signed or unsigned), and its bit / payload index
__device__ __forceinline__ bool perfect_index(uint64_t key, bool key_signed, int64_t min_value, uint64_t range, uint64_t &idx) {
	bool in_range;
	if (key_signed) {
		const int64_t v = (int64_t)key;
		in_range = v >= min_value && (uint64_t)(v - min_value) <= range;
		idx = (uint64_t)(v - min_value);
	} else {
		in_range = key >= (uint64_t)min_value && key - (uint64_t)min_value <= range;
		idx = key - (uint64_t)min_value;
	}
	return in_range;
}

// Hash tables are probed linearly, one aligned 32-byte slot group per round trip: a wave waits for its slowest lane, so
// what counts is the number of DEPENDENT loads of the unluckiest of 64 lanes; at load factor <= 0.5 a group of 4 (2)
// slots almost always holds the end of the probe sequence.  A group step inspects the slots of one group (a, b: its two
// 16-byte halves) from slot `first` on; the probe ends at an empty slot (a miss) or at the key.
// KIND_S8: {key32, row} x 4
__device__ __forceinline__ void s8_group_step(const uint4 a, const uint4 b, uint32_t first, uint32_t key, bool &searching,
                                              bool &hit, uint32_t &row) {
	const uint32_t kk[4] = {a.x, a.z, b.x, b.z};
	const uint32_t rr[4] = {a.y, a.w, b.y, b.w};
#pragma unroll
	for (int j = 0; j < 4; j++) {
		if (searching && (uint32_t)j >= first) {
			if (rr[j] == S8_EMPTY_ROW) {
				searching = false;
			} else if (kk[j] == key) {
				hit = true;
				row = rr[j];
				searching = false;
			}
		}
	}
}

// KIND_S16: {key64, start, count} x 2.  The key S16_EMPTY_KEY marks empty slots: its run is the table's side entry
// (sentinel_start, sentinel_count), found without a probe -- s16_begin_probe says whether a probe is needed
__device__ __forceinline__ void s16_begin_probe(uint64_t key, bool valid, uint32_t sentinel_start, uint32_t sentinel_count,
                                          bool &searching, uint32_t &start, uint32_t &count) {
	start = 0;
	count = 0;
	searching = valid;
	if (valid && key == S16_EMPTY_KEY) {
		start = sentinel_start;
		count = sentinel_count;
		searching = false;
	}
}
__device__ __forceinline__ void s16_group_step(const uint4 e0, const uint4 e1, uint32_t first, uint64_t key, bool &searching,
                                               uint32_t &start, uint32_t &count) {
	if (first == 0) {
		const uint64_t k0 = ((uint64_t)e0.y << 32) | e0.x;
		if (k0 == S16_EMPTY_KEY) {
			searching = false;
		} else if (k0 == key) {
			start = e0.z;
			count = e0.w;
			searching = false;
		}
	}
	if (searching) {
		const uint64_t k1 = ((uint64_t)e1.y << 32) | e1.x;
		if (k1 == S16_EMPTY_KEY) {
			searching = false;
		} else if (k1 == key) {
			start = e1.z;
			count = e1.w;
			searching = false;
		}
	}
}

// ---- output: a DevOut is a stream of chunks; a wave fills one chunk at a time
#define NO_CHUNK 0xFFFFFFFFu
struct OutState {
	uint32_t cur_chunk; // the chunk this wave fills, NO_CHUNK: none yet
	uint32_t fill;      // tuples in it
	bool emit;          // the current unit writes its final tuples
	bool overflow;      // the chunks ran out (cursor[1] is raised): nothing more is written
};
__device__ __forceinline__ OutState out_state_init() {
	return OutState {NO_CHUNK, 0u, false, false};
}
// the valid lanes of ballot `m` take consecutive places in the wave's chunks: `write(place)` stores this lane's tuple at
// `place` of every slot.  A full chunk leaves its fill in chunk_count[] and the next one is claimed at cursor[0]; when
// there are no more, cursor[1] is raised and the wave stops emitting
template <class WriteFn>
__device__ __forceinline__ void out_claim(const DevOut &out, OutState &os, uint32_t lane, uint64_t m, bool valid, WriteFn &&write) {
	const uint32_t n = (uint32_t)__popcll(m);
	const uint32_t rank = lane_rank(m);
	uint32_t done = 0;
	while (done < n) {
		if (os.cur_chunk == NO_CHUNK || os.fill == out.chunk_capacity) {
			if (os.cur_chunk != NO_CHUNK && lane == 0) {
				as_global(out.chunk_count)[os.cur_chunk] = os.fill;
			}
			uint32_t nc = 0;
			if (lane == 0) {
				nc = atomicAdd(&out.cursor[0], 1u);
			}
			nc = uni(nc);
			if (nc >= out.max_chunks) {
				if (lane == 0) {
					atomicExch(&out.cursor[1], 1u);
				}
				os.overflow = true;
				os.cur_chunk = NO_CHUNK;
				os.emit = false;
				return;
			}
			os.cur_chunk = nc;
			os.fill = 0;
		}
		const uint32_t room = out.chunk_capacity - os.fill;
		const uint32_t take = (n - done) < room ? (n - done) : room;
		if (valid && rank >= done && rank < done + take) {
			write((uint64_t)os.cur_chunk * out.chunk_capacity + os.fill + (rank - done));
		}
		os.fill += take;
		done += take;
	}
}
// the wave is done: its last chunk's fill
__device__ __forceinline__ void out_close(const DevOut &out, const OutState &os, uint32_t lane) {
	if (os.cur_chunk != NO_CHUNK && lane == 0) {
		as_global(out.chunk_count)[os.cur_chunk] = os.fill;
	}
}
#endif
