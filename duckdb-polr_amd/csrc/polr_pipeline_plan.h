// duckdb-polr_amd/csrc/polr_pipeline_plan.h -- what polr_pipeline_create decides, as plain host logic: which pipelines are
// refused (and with which words), which build ids a tuple carries, whether matches fold into multiplicities, where every
// key and condition operand is read from, and whether the counting variant runs on the flat kernel with which bit tables
// in LDS.  No HIP and no device memory in here: polr_capi.hip describes the handles in a PipePlanInput, calls
// polr_pipeline_plan() and writes the device structs from the answer; a stand-alone host program checks the rules against
// known answers and their invariants (tests/pipeplan/pipe_plan_main.cpp).
// The constants the plan shares with the device structs (polr_device.h) are defined here, once.
#pragma once

#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/polr_hip.h"

#define POLR_KMAX 8
#define POLR_PMAX 32
#define POLR_NKEYS 4
#define POLR_NPREDS 4

enum { KIND_NONE = 0, KIND_PERFECT = 1, KIND_S8 = 2, KIND_S16 = 3 };

static_assert(POLR_KMAX == POLR_MAX_JOINS, "device structs hold POLR_MAX_JOINS joins");
static_assert(POLR_PMAX == POLR_MAX_PATHS, "device structs hold POLR_MAX_PATHS join orders");
static_assert(POLR_NKEYS == POLR_MAX_KEYS, "device structs hold POLR_MAX_KEYS key columns");
static_assert(POLR_NPREDS == POLR_MAX_PREDS, "device structs hold POLR_MAX_PREDS conditions");

struct PipeCol {
	uint32_t width;
	uint32_t sx; // signed: sign-extended when it is widened
};

// one join: what the plan needs of the build side (polr_ht), and the caller's descriptor
struct PipePlanJoin {
	uint32_t kind; // KIND_NONE: no handle, or not finalized (nothing else is read then)
	uint32_t n_keys;
	uint32_t key_width[POLR_NKEYS], key_flags[POLR_NKEYS]; // (flags: POLR_KEY_*)
	uint32_t key_signed;
	std::vector<PipeCol> cols; // payload columns as the kernels read them
	uint64_t capacity, max_run;
	int64_t min_value, max_value;
	uint64_t range;
	uint32_t packed; // composite key in packed form (KeyPack)
	int device;
	const void *table; // identity only: the same build side joined twice shares one LDS copy
	polr_join_desc desc; // (desc.ht is never followed)
};

struct PipePlanInput {
	std::vector<PipeCol> probe_cols;
	uint64_t n_probe_rows;
	int device; // of the context
	uint32_t k, n_paths;
	std::vector<PipePlanJoin> joins; // [k] (may be empty when k is outside 1..POLR_MAX_JOINS: refused before a join is read)
	const int32_t *paths;            // [n_paths][k]
	size_t flat_wave_bytes;          // polr_pool_flat_wave_bytes(k): LDS one wave of the flat kernel takes for its queues
};

// where a key or the left side of a condition is read from
struct PipeSource {
	int32_t join; // -1: the probe table
	int32_t col;
	uint32_t width, sx;
};

struct PipeSlots {
	uint32_t W;                      // slots per tuple: 1 (probe row) + carried build ids
	int32_t slot_of_join[POLR_KMAX]; // slot of join j's build id, -1: not carried
};

struct PipePlan {
	int code; // POLR_OK, or why the pipeline is refused: msg is the text
	char msg[512];
	PipeSlots mat, count; // materialising variant (slot 1 + j = join j) and counting variant
	uint32_t mult;        // counting variant: some join's matches fold into multiplicities (polr_gen_device.h)
	struct Join {
		uint32_t unique; // 1: at most one build row per key; 2: keys may repeat
		uint32_t ext;    // its stages need an extension record (packed composite key, non-equality conditions)
		PipeSource key[POLR_NKEYS], pred[POLR_NPREDS];
		uint32_t lds_off1; // flat: 1 + dword offset of its bit table in the LDS table area; 0: read from HBM
	} joins[POLR_KMAX];
	// flat pipelines (polr_flat_device.h)
	uint32_t flat, flat_emit, flat_wpb; // counting variant may run flat; emitting runs too; waves per workgroup
	uint32_t n_lds_tables, lds_table_dwords;
	uint32_t lds_table_join[POLR_KMAX]; // a join whose bit table is LDS table t
	uint32_t lds_table_off[POLR_KMAX], lds_table_len[POLR_KMAX]; // dwords
};

#if defined(__GNUC__)
__attribute__((format(printf, 3, 4)))
#endif
static inline int pipe_plan_refuse(PipePlan &pl, int code, const char *fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(pl.msg, sizeof(pl.msg), fmt, ap);
	va_end(ap);
	pl.code = code;
	return code;
}

// a cell the kernels widen to 64 bits (load_cell)
static inline bool pipe_int_width(uint32_t w) {
	return w == 1 || w == 2 || w == 4 || w == 8;
}

// Can a column of `probe_width` bytes be compared with a build key of `build_width` bytes that carries `build_flags`
// (POLR_KEY_*)?  JoinHashTable asserts left/right key types equal (join_hashtable.cpp:24): the reference's left side is then
// CAST(column) (polar_config.cpp:75-82).  An integer cast is a comparison by VALUE, which a table whose key column carries
// POLR_KEY_BY_VALUE does on the device -- no materialised copy of the probe column.  The one rule behind a join's keys
// (pipe_plan_validate) and the columns of a SEMI / ANTI filter (polr_htsemi_plan.h); each caller words its own refusal.
enum { PIPE_KEYS_PAIR = 0, PIPE_KEYS_WIDTHS_DIFFER = 1, PIPE_KEYS_NO_INTEGER = 2 };
static inline int pipe_key_pairing(uint32_t probe_width, uint32_t build_width, uint32_t build_flags) {
	if (probe_width != build_width && !(build_flags & POLR_KEY_BY_VALUE)) {
		return PIPE_KEYS_WIDTHS_DIFFER;
	}
	return pipe_int_width(probe_width) ? PIPE_KEYS_PAIR : PIPE_KEYS_NO_INTEGER;
}

// the join (-1: the probe table) source c of a join reads: its keys first, then the left sides of its conditions
static inline int32_t pipe_src_join(const polr_join_desc &d, uint32_t c) {
	return c < d.n_keys ? d.key_src_join[c] : d.pred_src_join[c - d.n_keys];
}

// column (sj, sc) a key or a condition (`what`) of join j reads; sj is in range and not j (checked before)
static inline int pipe_plan_resolve(const PipePlanInput &in, PipePlan &pl, uint32_t j, const char *what, uint32_t c,
                                    int32_t sj, int32_t sc, PipeSource &s) {
	const std::vector<PipeCol> &cols = sj < 0 ? in.probe_cols : in.joins[sj].cols;
	if (sc < 0 || (size_t)sc >= cols.size()) {
		if (sj < 0) {
			return pipe_plan_refuse(pl, POLR_E_INVALID, "join %u %s %u: probe column %d out of range", j, what, c, sc);
		}
		return pipe_plan_refuse(pl, POLR_E_INVALID, "join %u %s %u: build column (%d,%d) out of range", j, what, c, sj, sc);
	}
	s.join = sj < 0 ? -1 : sj;
	s.col = sc;
	s.width = cols[sc].width;
	s.sx = cols[sc].sx;
	return POLR_OK;
}

static inline int pipe_plan_validate(const PipePlanInput &in, PipePlan &pl) {
	const uint32_t k = in.k, n_paths = in.n_paths;
	if (k < 1 || k > POLR_MAX_JOINS) {
		return pipe_plan_refuse(pl, POLR_E_UNSUPPORTED, "%u multiplexed joins not supported (1..%d)", k, POLR_MAX_JOINS);
	}
	if (n_paths < 1 || n_paths > POLR_MAX_PATHS) {
		return pipe_plan_refuse(pl, POLR_E_UNSUPPORTED, "%u join orders not supported (1..%d)", n_paths, POLR_MAX_PATHS);
	}
	if (in.n_probe_rows >= 0xFFFFFFF0ull) {
		return pipe_plan_refuse(pl, POLR_E_UNSUPPORTED, "probe side of %llu rows exceeds the 32-bit row-id space per shard",
		                        (unsigned long long)in.n_probe_rows);
	}
	// the descriptors first: the dependency walk below reads n_keys / n_preds entries of every join and shifts by the
	// join index a key or a condition names
	for (uint32_t j = 0; j < k; j++) {
		const PipePlanJoin &t = in.joins[j];
		const polr_join_desc &d = t.desc;
		if (t.kind == KIND_NONE) {
			return pipe_plan_refuse(pl, POLR_E_INVALID, "join %u: build side not finalized", j);
		}
		if (d.n_keys != t.n_keys || d.n_keys < 1 || d.n_keys > POLR_MAX_KEYS) {
			return pipe_plan_refuse(pl, POLR_E_INVALID, "join %u: %u probe keys for a %u-key table", j, d.n_keys, t.n_keys);
		}
		if (d.n_preds > POLR_MAX_PREDS) {
			return pipe_plan_refuse(pl, POLR_E_UNSUPPORTED, "join %u: %u non-equality conditions (at most %d)", j, d.n_preds,
			                        POLR_MAX_PREDS);
		}
		for (uint32_t c = 0; c < d.n_keys + d.n_preds; c++) {
			const int32_t sj = pipe_src_join(d, c);
			if (sj >= 0 && ((uint32_t)sj >= k || (uint32_t)sj == j)) {
				return pipe_plan_refuse(pl, POLR_E_INVALID, "join %u %s %u: reads a build column of join %d", j,
				                        c < d.n_keys ? "key" : "condition", c < d.n_keys ? c : c - d.n_keys, sj);
			}
		}
	}
	// every path must be a permutation of 0..k-1 that respects the key dependencies
	// (POLARConfig join_prerequisites, polar_config.cpp:72-95)
	for (uint32_t p = 0; p < n_paths; p++) {
		uint32_t seen = 0;
		for (uint32_t j = 0; j < k; j++) {
			const int32_t x = in.paths[p * k + j];
			if (x < 0 || (uint32_t)x >= k || (seen >> x) & 1) {
				return pipe_plan_refuse(pl, POLR_E_INVALID, "path %u is not a permutation of the %u joins", p, k);
			}
			const polr_join_desc &d = in.joins[x].desc;
			for (uint32_t c = 0; c < d.n_keys + d.n_preds; c++) {
				const int32_t sj = pipe_src_join(d, c);
				if (sj >= 0 && !((seen >> sj) & 1)) {
					return pipe_plan_refuse(pl, POLR_E_INVALID, "path %u probes join %d before join %d that %s", p, x, sj,
					                        c < d.n_keys ? "provides its key" : "a condition of it reads");
				}
			}
			seen |= 1u << x;
		}
	}
	// the columns: where every key and condition operand is read from, and that the two sides can be compared
	for (uint32_t j = 0; j < k; j++) {
		const PipePlanJoin &t = in.joins[j];
		const polr_join_desc &d = t.desc;
		if (t.device != in.device) {
			return pipe_plan_refuse(pl, POLR_E_INVALID, "join %u: build side lives on another device", j);
		}
		for (uint32_t c = 0; c < d.n_keys; c++) {
			PipeSource &s = pl.joins[j].key[c];
			if (pipe_plan_resolve(in, pl, j, "key", c, d.key_src_join[c], d.key_src_col[c], s)) {
				return pl.code;
			}
			const int pairing = pipe_key_pairing(s.width, t.key_width[c], t.key_flags[c]);
			if (pairing == PIPE_KEYS_WIDTHS_DIFFER) {
				return pipe_plan_refuse(pl, POLR_E_INVALID,
				                        "join %u key %u: probe key is %u bytes, build key %u bytes (a CAST'ed key: "
				                        "polr_ht_set_key_flags(..., POLR_KEY_BY_VALUE) before the table is finalized)",
				                        j, c, s.width, t.key_width[c]);
			}
			if (pairing == PIPE_KEYS_NO_INTEGER) {
				return pipe_plan_refuse(pl, POLR_E_UNSUPPORTED, "join %u key %u: probe key of %u bytes", j, c, s.width);
			}
		}
		for (uint32_t c = 0; c < d.n_preds; c++) {
			const uint32_t bc = d.pred_build_col[c];
			const uint32_t op = d.pred_op[c];
			if (op > POLR_CMP_GE && op != POLR_CMP_STR_EQ) {
				return pipe_plan_refuse(pl, POLR_E_UNSUPPORTED,
				                        "join %u condition %u: comparison %u (EQ, NE, LT, GT, LE, GE, STR_EQ)", j, c, op);
			}
			if (bc >= t.cols.size()) {
				return pipe_plan_refuse(pl, POLR_E_INVALID, "join %u condition %u: build column %u out of range", j, c, bc);
			}
			PipeSource &s = pl.joins[j].pred[c];
			if (pipe_plan_resolve(in, pl, j, "condition", c, d.pred_src_join[c], d.pred_src_col[c], s)) {
				return pl.code;
			}
			const uint32_t bwidth = t.cols[bc].width;
			if (op == POLR_CMP_STR_EQ) {
				if (s.width != 16 || bwidth != 16) {
					return pipe_plan_refuse(pl, POLR_E_INVALID,
					                        "join %u condition %u: STR_EQ compares two columns of 16-byte string cells "
					                        "(left %u bytes, right %u bytes)",
					                        j, c, s.width, bwidth);
				}
			} else if (s.width != bwidth || !pipe_int_width(s.width)) {
				return pipe_plan_refuse(pl, POLR_E_INVALID, "join %u condition %u: left side is %u bytes, right side %u bytes", j,
				                        c, s.width, bwidth);
			}
		}
	}
	return POLR_OK;
}

// Flat pipelines (polr_flat_device.h): every join keyed by ONE 4-byte probe column, at most one build row per key
// (perfect bit table or unique-key hash table).  Decides the workgroup shape of the flat pool kernel and which bit
// tables stay in LDS for the whole run (smallest first, while they fit beside the per-wave queues).
static inline void pipe_plan_flat(const PipePlanInput &in, PipePlan &pl) {
	const uint32_t k = in.k;
	if (pl.count.W != 1 || k > 6) {
		return; // some join reads its key through a build column / more joins than the sweep holds in registers
	}
	for (uint32_t j = 0; j < k; j++) {
		const PipePlanJoin &t = in.joins[j];
		if (t.n_keys != 1 || t.desc.key_src_join[0] >= 0 || t.key_width[0] != 4 || t.desc.n_preds != 0) {
			return;
		}
		if (t.kind == KIND_PERFECT) {
			// the flat lookup works in 32-bit modular arithmetic: [min, max] must lie inside the key type's domain
			const int64_t lo = t.key_signed ? -2147483648ll : 0ll;
			const int64_t hi = t.key_signed ? 2147483647ll : 4294967295ll;
			if (t.min_value < lo || t.max_value > hi || t.range > 0xFFFFFFFFull) {
				return;
			}
		} else if (t.kind != KIND_S8 || t.capacity > (1ull << 31)) {
			return;
		}
	}
	const size_t per_wave = in.flat_wave_bytes;
	uint32_t wpb = 4;
	for (uint32_t w : {16u, 8u}) {
		if (per_wave * w <= 120u * 1024) {
			wpb = w;
			break;
		}
	}
	pl.flat_wpb = wpb;
	// one workgroup of 16 waves per CU leaves the rest of the 160 KB to the tables; smaller workgroups share a CU
	const size_t budget = wpb == 16 ? std::min<size_t>(64u * 1024, 156u * 1024 - per_wave * wpb) : 16u * 1024;
	std::vector<uint32_t> order;
	for (uint32_t j = 0; j < k; j++) {
		if (in.joins[j].kind == KIND_PERFECT) {
			order.push_back(j);
		}
	}
	std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return in.joins[a].range < in.joins[b].range; });
	uint32_t used = 0;
	for (uint32_t j : order) {
		const PipePlanJoin &t = in.joins[j];
		const uint32_t words = (uint32_t)((t.range + 1 + 31) / 32);
		// the same build side joined twice shares one LDS copy
		bool shared = false;
		for (uint32_t x = 0; x < pl.n_lds_tables; x++) {
			if (in.joins[pl.lds_table_join[x]].table == t.table) {
				pl.joins[j].lds_off1 = pl.lds_table_off[x] + 1;
				shared = true;
			}
		}
		if (shared) {
			continue;
		}
		const uint32_t padded = (words + 3u) & ~3u;
		if (((size_t)used + padded) * 4 > budget || pl.n_lds_tables >= POLR_KMAX) {
			break;
		}
		pl.lds_table_join[pl.n_lds_tables] = j;
		pl.lds_table_off[pl.n_lds_tables] = used;
		pl.lds_table_len[pl.n_lds_tables] = words;
		pl.n_lds_tables++;
		pl.joins[j].lds_off1 = used + 1;
		used += padded;
	}
	pl.lds_table_dwords = used;
	// (an emitting run needs every join's build id: a perfect table's is the key's offset, a hash table's would take a
	// second probe -- such banks emit through the generic pipeline)
	pl.flat_emit = order.size() == k;
	pl.flat = 1;
}

// returns pl.code
static inline int polr_pipeline_plan(const PipePlanInput &in, PipePlan &pl) {
	pl = PipePlan();
	if (pipe_plan_validate(in, pl)) {
		return pl.code;
	}
	const uint32_t k = in.k;
	// materialising variant: slot 1+j = join j (the adaptive union's column order)
	pl.mat.W = 1 + k;
	for (uint32_t j = 0; j < POLR_KMAX; j++) {
		pl.mat.slot_of_join[j] = j < k ? (int32_t)(1 + j) : -1;
		pl.count.slot_of_join[j] = -1;
	}
	// counting variant: carry only the build ids some later join reads its key (or a condition's left side) through
	uint32_t w = 1;
	for (uint32_t j = 0; j < k; j++) {
		const polr_join_desc &d = in.joins[j].desc;
		for (uint32_t c = 0; c < d.n_keys + d.n_preds; c++) {
			const int32_t sj = pipe_src_join(d, c);
			if (sj >= 0 && pl.count.slot_of_join[sj] < 0) {
				pl.count.slot_of_join[sj] = (int32_t)w++;
			}
		}
	}
	pl.count.W = w;
	// multiplicities (polr_gen_device.h): worth a tuple slot when some join's matches can be folded into them -- its
	// build key may repeat, nobody reads its build rows downstream, it has no non-equality condition
	for (uint32_t j = 0; j < k; j++) {
		const PipePlanJoin &t = in.joins[j];
		// 1: at most one match per tuple; 2: keys may repeat (wide steps fall back to a narrow one where they do)
		pl.joins[j].unique = (t.kind == KIND_PERFECT || t.kind == KIND_S8 || t.max_run <= 1) ? 1u : 2u;
		pl.joins[j].ext = (t.packed || t.desc.n_preds) ? 1u : 0u;
		if (pl.joins[j].unique == 2 && pl.count.slot_of_join[j] < 0 && t.desc.n_preds == 0) {
			pl.mult = 1;
		}
	}
	pipe_plan_flat(in, pl);
	return POLR_OK;
}
