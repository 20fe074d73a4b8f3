// duckdb-polr_amd/csrc/polr_agg_plan.h -- the contract of the aggregate sinks (polr_out_aggregate*, polr_out_fuse_grouped;
// include/polr_hip.h), as plain host code.  No HIP in here: polr_agg.hip resolves the columns a request names, describes them,
// and builds its device structs from what the plan says; polr_fuseagg_plan.h takes the argument rule and the decode from
// here; a stand-alone host program drives the header alone (tests/aggplan/agg_plan_main.cpp).
//
// Every refusal, in this order, each with its message (a refusal "without message" leaves err empty: the caller returns the
// code and leaves the context's error as it was):
//
//   polr_agg_plan_ungrouped      polr_out_aggregate, polr_out_aggregate_expr
//     1. NULL output, specs or results; no aggregates                         POLR_E_INVALID, without message
//     2. the output holds aggregate cells (a fused ungrouped sink)            POLR_E_INVALID
//     3. more than POLR_AGG_MAX_AGGS aggregates                               POLR_E_UNSUPPORTED
//     4. per aggregate, in order: the argument rule (below)
//
//   polr_agg_plan_grouped        polr_out_aggregate_grouped, polr_out_aggregate_grouped_expr
//     1. NULL output, keys, specs or results; no group columns or aggregates  POLR_E_INVALID, without message
//     2. the output holds aggregate cells                                     POLR_E_INVALID
//     3. more than 3 group columns or 8 aggregates                            POLR_E_UNSUPPORTED
//     4. per group column, in order: the perfect-domain rule (below), limit 2^20
//     5. the results hold another number of groups than the domains span      POLR_E_INVALID
//     6. per aggregate, in order: the argument rule
//
//   polr_agg_plan_hashed         polr_out_aggregate_hashed, _hashed_str, _hashed_expr
//     1. NULL output, cols, specs, group_keys, group_nulls, results or n_groups; no group columns or aggregates;
//        max_groups == 0; strings allowed and NULL str_used, or NULL str_bytes with str_cap > 0
//                                                                             POLR_E_INVALID, without message
//     2. the output holds aggregate cells                                     POLR_E_INVALID
//     3. more than 3 group columns, 8 aggregates or 2^24 groups               POLR_E_UNSUPPORTED
//        (from here on *str_used is 0 whatever follows: head_passed)
//     4. per group column, in order: out of range (POLR_E_INVALID); a 16-byte column is a string column where the call
//        allows strings (its bit of str_mask), every other column falls under the integer rule (POLR_E_UNSUPPORTED)
//     5. per aggregate, in order: the argument rule
//
//   polr_agg_plan_fuse_grouped   polr_out_fuse_grouped
//     1. NULL output                                                          POLR_E_INVALID, without message
//        (keys == NULL or n_keys == 0: un-fuse, never refused)
//     2. NULL specs, no aggregates, more than 3 group columns or 8 aggregates POLR_E_INVALID
//     3. not a flat emitting pipeline                                         POLR_E_UNSUPPORTED
//     4. the output carries a fused sink already (either kind)                POLR_E_INVALID
//     5. per group column, in order: the perfect-domain rule, limit 4096
//     6. per aggregate, in order: a function other than COUNT(*), COUNT and SUM (POLR_E_UNSUPPORTED, before "unknown
//        function"); the argument rule; a SUM over a column wider than 4 bytes (POLR_E_UNSUPPORTED)
//
//   the argument rule (polr_agg_arg_rule), for the column form (polr_agg_spec: op = POLR_ARG_COLUMN) and the expression
//   form (polr_agg_expr):
//     an unknown function                                                     POLR_E_INVALID
//     (COUNT(*): nothing else is looked at)
//     an unknown operator                                                     POLR_E_INVALID
//     per operand, left then right: out of range (POLR_E_INVALID; "probe column c" or "build column (j,c)"); the integer
//     rule: up to 8 bytes, signed if 8 (POLR_E_UNSUPPORTED)
//     (POLR_ARG_COLUMN: nothing else is looked at)
//     a result width other than 1, 2, 4, 8                                    POLR_E_INVALID
//     an unsigned 8-byte result                                               POLR_E_UNSUPPORTED
//     a result type that cannot hold an operand type, left then right         POLR_E_INVALID
//     -> lo, hi: the bounds of the result type
//
//   the perfect-domain rule (polr_agg_perfect_domains), per group column: out of range (POLR_E_INVALID); the integer rule
//   (POLR_E_UNSUPPORTED); an empty domain -- the perfect-hash sink: POLR_E_INVALID "empty domain", the fused sink:
//   POLR_E_UNSUPPORTED with its 4096 message; the running product of the domains above the limit -- POLR_E_UNSUPPORTED, each
//   sink with its own text.
//
// Besides: polr_hashagg_layout (the hashed sink's one allocation), polr_agg_decode (an accumulated aggregate as the C ABI
// reports it) and polr_fused_group_words (the fused GROUP BY sink's 64-bit words per group).
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/polr_hip.h"

#define POLR_AGG_MAX_AGGS 8u       // (= POLR_MAX_AGGS, POLR_MAX_GROUP_KEYS of polr_device.h: static_assert in polr_agg.hip)
#define POLR_AGG_MAX_GROUP_KEYS 3u
#define POLR_AGG_PERFECT_GROUPS (1ull << 20) // the perfect-hash sink's groups
#define POLR_AGG_FUSED_GROUPS 4096ull        // the fused GROUP BY sink's
#define POLR_AGG_HASHED_GROUPS (1ull << 24)  // the hashed sink's max_groups

struct PolrAggCol { // a column a request names, described
	bool in_range;         // (src_join, src_col) names a column of the pipeline
	uint32_t width, flags; // of that column (flags: POLR_COL_SIGNED)
};
struct PolrAggArg { // one aggregate as requested -- the column form is op = POLR_ARG_COLUMN --, its operand columns described
	uint32_t fn, op;
	int32_t src_join[2];
	uint32_t src_col[2];
	uint32_t result_width, result_flags;
	PolrAggCol col[2];
};
struct PolrAggArgPlan { // ... and as the sink kernels take it
	uint32_t fn, op;
	long long lo, hi; // the range of the declared result type (0, 0 for POLR_ARG_COLUMN)
};
struct PolrAggGroupCol {
	int32_t src_join;
	uint32_t src_col;
	uint32_t n_values; // (the hashed sink ignores it)
	PolrAggCol col;
};
struct PolrAggRequest {
	bool has_out, has_specs, has_results;
	bool agg_cells;         // the output carries a fused ungrouped sink: it holds aggregate cells, no row ids
	uint32_t n_aggs;
	const PolrAggArg *args; // [n_aggs] (read only when the counts are in range)
	// the grouped sinks
	bool has_keys;
	uint32_t n_keys;
	const PolrAggGroupCol *keys; // [n_keys] (as args)
	uint64_t n_groups;           // the perfect-hash sink: what the results hold
	// the hashed sink
	bool has_group_outputs; // group_keys, group_nulls and n_groups
	uint64_t max_groups;
	bool strings, has_str_used, has_str_bytes;
	uint64_t str_cap;
	// polr_out_fuse_grouped
	bool flat_emit;     // a flat pipeline whose emitting runs take the flat kernel
	bool already_fused; // the output carries a grouped or an ungrouped fused sink
};
struct PolrAggPlan {
	char err[256];
	uint32_t n_aggs;
	PolrAggArgPlan agg[POLR_AGG_MAX_AGGS];
	uint64_t n_groups; // the perfect-hash and the fused sink: the product of the domains
	uint32_t str_mask; // the hashed sink: bit q = group column q holds strings
	bool head_passed;  // the hashed sink: refusals 1-3 did not apply
	bool unfuse;       // polr_out_fuse_grouped: detach, nothing else is set
};

#define POLR_AP_REFUSE(code_, ...)                                                                                     \
	do {                                                                                                               \
		snprintf(err, 256, __VA_ARGS__);                                                                               \
		return (code_);                                                                                                \
	} while (0)

// the fused GROUP BY sink's 64-bit words per group: the rows of the group, and per aggregate its sum and its count
static inline uint32_t polr_fused_group_words(uint32_t n_aggs) {
	return 1u + 2u * n_aggs;
}

// the refusal of a column out of range ("<what> <idx>: ..."), in the wording of its side
static inline int polr_agg_col_out_of_range(int32_t src_join, uint32_t src_col, const char *what, uint32_t idx, char *err) {
	if (src_join < 0) {
		POLR_AP_REFUSE(POLR_E_INVALID, "%s %u: probe column %u out of range", what, idx, src_col);
	}
	POLR_AP_REFUSE(POLR_E_INVALID, "%s %u: build column (%d,%u) out of range", what, idx, src_join, src_col);
}

// a column a cell-valued sink reads: in range, and an integer of up to 8 bytes (signed if 8)
static inline int polr_agg_int_col(const PolrAggCol &c, int32_t src_join, uint32_t src_col, const char *what, uint32_t idx,
                                   char *err) {
	if (!c.in_range) {
		return polr_agg_col_out_of_range(src_join, src_col, what, idx, err);
	}
	if (c.width > 8 || (c.width == 8 && !(c.flags & POLR_COL_SIGNED))) {
		POLR_AP_REFUSE(POLR_E_UNSUPPORTED, "%s %u: only integer columns of up to 8 bytes (signed if 8)", what, idx);
	}
	return POLR_OK;
}

static inline PolrAggArg polr_agg_arg_of(const polr_agg_spec &s) {
	PolrAggArg g;
	memset(&g, 0, sizeof(g));
	g.fn = s.fn;
	g.op = POLR_ARG_COLUMN;
	g.src_join[0] = s.src_join;
	g.src_col[0] = s.src_col;
	return g;
}
static inline PolrAggArg polr_agg_arg_of(const polr_agg_expr &s) {
	PolrAggArg g;
	memset(&g, 0, sizeof(g));
	g.fn = s.fn;
	g.op = s.op;
	for (uint32_t x = 0; x < 2; x++) {
		g.src_join[x] = s.src_join[x];
		g.src_col[x] = s.src_col[x];
	}
	g.result_width = s.result_width;
	g.result_flags = s.result_flags;
	return g;
}
// the operands of an accepted aggregate whose columns the sink reads
static inline uint32_t polr_agg_n_operands(const PolrAggArgPlan &ap) {
	return ap.fn == POLR_AGG_COUNT_STAR ? 0u : (ap.op == POLR_ARG_COLUMN ? 1u : 2u);
}

// aggregate `a` of a call, in either form -> POLR_OK with *ap filled, or the first refusal with err set
static inline int polr_agg_arg_rule(const PolrAggArg &g, uint32_t a, PolrAggArgPlan *ap, char *err) {
	memset(ap, 0, sizeof(*ap));
	if (g.fn > POLR_AGG_MAX) {
		POLR_AP_REFUSE(POLR_E_INVALID, "aggregate %u: unknown function %u", a, g.fn);
	}
	ap->fn = g.fn;
	ap->op = POLR_ARG_COLUMN;
	if (g.fn == POLR_AGG_COUNT_STAR) {
		return POLR_OK;
	}
	if (g.op > POLR_ARG_MUL) {
		POLR_AP_REFUSE(POLR_E_INVALID, "aggregate %u: unknown operator %u", a, g.op);
	}
	ap->op = g.op;
	for (uint32_t x = 0; x < polr_agg_n_operands(*ap); x++) {
		if (const int rc = polr_agg_int_col(g.col[x], g.src_join[x], g.src_col[x], "aggregate", a, err)) {
			return rc;
		}
	}
	if (g.op == POLR_ARG_COLUMN) {
		return POLR_OK;
	}
	const uint32_t rw = g.result_width;
	const bool rsigned = (g.result_flags & POLR_COL_SIGNED) != 0;
	if (rw != 1 && rw != 2 && rw != 4 && rw != 8) {
		POLR_AP_REFUSE(POLR_E_INVALID, "aggregate %u: result width %u (1, 2, 4 or 8 bytes)", a, rw);
	}
	if (rw == 8 && !rsigned) {
		POLR_AP_REFUSE(POLR_E_UNSUPPORTED, "aggregate %u: an 8-byte result type must be signed", a);
	}
	for (uint32_t x = 0; x < 2; x++) { // (lossless implicit casts only: same signedness and no narrower, or unsigned into a wider signed)
		const uint32_t w = g.col[x].width;
		const bool sgn = (g.col[x].flags & POLR_COL_SIGNED) != 0;
		const bool holds = sgn == rsigned ? w <= rw : (!sgn && w < rw);
		if (!holds) {
			POLR_AP_REFUSE(POLR_E_INVALID, "aggregate %u: a %ssigned %u-byte result cannot hold every value of its %s operand (%ssigned, %u bytes)",
			               a, rsigned ? "" : "un", rw, x ? "right" : "left", sgn ? "" : "un", w);
		}
	}
	if (rsigned) {
		ap->hi = (long long)(0x7FFFFFFFFFFFFFFFull >> (64u - 8u * rw));
		ap->lo = -ap->hi - 1;
	} else {
		ap->lo = 0;
		ap->hi = (long long)(0xFFFFFFFFFFFFFFFFull >> (64u - 8u * rw));
	}
	return POLR_OK;
}

static inline int polr_agg_args(const PolrAggRequest &rq, PolrAggPlan *pl) {
	pl->n_aggs = rq.n_aggs;
	for (uint32_t a = 0; a < rq.n_aggs; a++) {
		if (const int rc = polr_agg_arg_rule(rq.args[a], a, &pl->agg[a], pl->err)) {
			return rc;
		}
	}
	return POLR_OK;
}

// group columns with small dense domains, of the perfect-hash sink or (fused) of the fused GROUP BY sink -> *n_groups, the
// product of the domains.  (The running product is at most the limit before a domain below 2^32 multiplies it: no wrap.)
static inline int polr_agg_perfect_domains(const PolrAggGroupCol *keys, uint32_t n_keys, bool fused, uint64_t *n_groups, char *err) {
	uint64_t groups = 1;
	for (uint32_t q = 0; q < n_keys; q++) {
		if (const int rc = polr_agg_int_col(keys[q].col, keys[q].src_join, keys[q].src_col, "group column", q, err)) {
			return rc;
		}
		groups *= keys[q].n_values;
		if (fused) {
			if (keys[q].n_values == 0 || groups > POLR_AGG_FUSED_GROUPS) {
				POLR_AP_REFUSE(POLR_E_UNSUPPORTED, "group column %u: a fused sink holds at most 4096 groups", q);
			}
			continue;
		}
		if (keys[q].n_values == 0) {
			POLR_AP_REFUSE(POLR_E_INVALID, "group column %u: empty domain", q);
		}
		if (groups > POLR_AGG_PERFECT_GROUPS) {
			POLR_AP_REFUSE(POLR_E_UNSUPPORTED, "more than 2^20 groups: not a perfect-hash aggregate");
		}
	}
	*n_groups = groups;
	return POLR_OK;
}

#define POLR_AP_HEAD(pl_)                                                                                              \
	memset((pl_), 0, sizeof(*(pl_)));                                                                                  \
	char *const err = (pl_)->err
// (the text of POLR_REFUSE_AGG_CELLS, polr_internal.h, too: every call that reads row ids refuses such an output)
#define POLR_AGG_CELLS_TEXT "the output has a fused aggregate sink: it holds aggregate cells, no row ids (polr_out_fused_aggregate_result)"
#define POLR_AP_REFUSE_AGG_CELLS(rq_)                                                                                  \
	if ((rq_).agg_cells) {                                                                                             \
		POLR_AP_REFUSE(POLR_E_INVALID, POLR_AGG_CELLS_TEXT);                                                           \
	}

static inline int polr_agg_plan_ungrouped(const PolrAggRequest &rq, PolrAggPlan *pl) {
	POLR_AP_HEAD(pl);
	if (!rq.has_out || !rq.has_specs || !rq.has_results || rq.n_aggs == 0) {
		return POLR_E_INVALID;
	}
	POLR_AP_REFUSE_AGG_CELLS(rq);
	if (rq.n_aggs > POLR_AGG_MAX_AGGS) {
		POLR_AP_REFUSE(POLR_E_UNSUPPORTED, "at most %d aggregates per call", (int)POLR_AGG_MAX_AGGS);
	}
	return polr_agg_args(rq, pl);
}

static inline int polr_agg_plan_grouped(const PolrAggRequest &rq, PolrAggPlan *pl) {
	POLR_AP_HEAD(pl);
	if (!rq.has_out || !rq.has_keys || !rq.has_specs || !rq.has_results || rq.n_keys == 0 || rq.n_aggs == 0) {
		return POLR_E_INVALID;
	}
	POLR_AP_REFUSE_AGG_CELLS(rq);
	if (rq.n_keys > POLR_AGG_MAX_GROUP_KEYS || rq.n_aggs > POLR_AGG_MAX_AGGS) {
		POLR_AP_REFUSE(POLR_E_UNSUPPORTED, "at most %d group columns and %d aggregates", (int)POLR_AGG_MAX_GROUP_KEYS,
		               (int)POLR_AGG_MAX_AGGS);
	}
	if (const int rc = polr_agg_perfect_domains(rq.keys, rq.n_keys, false, &pl->n_groups, err)) {
		return rc;
	}
	if (pl->n_groups != rq.n_groups) {
		POLR_AP_REFUSE(POLR_E_INVALID, "results hold %llu groups, the domains span %llu", (unsigned long long)rq.n_groups,
		               (unsigned long long)pl->n_groups);
	}
	return polr_agg_args(rq, pl);
}

static inline int polr_agg_plan_hashed(const PolrAggRequest &rq, PolrAggPlan *pl) {
	POLR_AP_HEAD(pl);
	if (!rq.has_out || !rq.has_keys || !rq.has_specs || !rq.has_group_outputs || !rq.has_results || rq.n_keys == 0 ||
	    rq.n_aggs == 0 || rq.max_groups == 0 || (rq.strings && (!rq.has_str_used || (!rq.has_str_bytes && rq.str_cap)))) {
		return POLR_E_INVALID;
	}
	POLR_AP_REFUSE_AGG_CELLS(rq);
	if (rq.n_keys > POLR_AGG_MAX_GROUP_KEYS || rq.n_aggs > POLR_AGG_MAX_AGGS || rq.max_groups > POLR_AGG_HASHED_GROUPS) {
		POLR_AP_REFUSE(POLR_E_UNSUPPORTED, "at most %d group columns, %d aggregates and 2^24 groups", (int)POLR_AGG_MAX_GROUP_KEYS,
		               (int)POLR_AGG_MAX_AGGS);
	}
	pl->head_passed = true;
	for (uint32_t q = 0; q < rq.n_keys; q++) {
		const PolrAggGroupCol &k = rq.keys[q];
		if (k.col.in_range && rq.strings && k.col.width == 16) {
			pl->str_mask |= 1u << q;
		} else if (const int rc = polr_agg_int_col(k.col, k.src_join, k.src_col, "group column", q, err)) {
			return rc;
		}
	}
	return polr_agg_args(rq, pl);
}

static inline int polr_agg_plan_fuse_grouped(const PolrAggRequest &rq, PolrAggPlan *pl) {
	POLR_AP_HEAD(pl);
	if (!rq.has_out) {
		return POLR_E_INVALID;
	}
	if (!rq.has_keys || rq.n_keys == 0) {
		pl->unfuse = true;
		return POLR_OK;
	}
	if (!rq.has_specs || rq.n_aggs == 0 || rq.n_keys > POLR_AGG_MAX_GROUP_KEYS || rq.n_aggs > POLR_AGG_MAX_AGGS) {
		POLR_AP_REFUSE(POLR_E_INVALID, "1..%d group columns and 1..%d aggregates", (int)POLR_AGG_MAX_GROUP_KEYS, (int)POLR_AGG_MAX_AGGS);
	}
	if (!rq.flat_emit) {
		POLR_AP_REFUSE(POLR_E_UNSUPPORTED,
		               "a GROUP BY sink is fused into FLAT pipelines whose joins are all perfect tables (polr_pipeline_launch_info); "
		               "others: polr_out_aggregate_grouped over the emitted row ids");
	}
	if (rq.already_fused) { // (at most one of the two sinks: polr_out_fuse_aggregate)
		POLR_AP_REFUSE(POLR_E_INVALID, "the output object already has a fused sink");
	}
	if (const int rc = polr_agg_perfect_domains(rq.keys, rq.n_keys, true, &pl->n_groups, err)) {
		return rc;
	}
	pl->n_aggs = rq.n_aggs;
	for (uint32_t a = 0; a < rq.n_aggs; a++) { // (per aggregate, in this order: the first refusal decides the return code)
		const PolrAggArg &g = rq.args[a];
		if (g.fn > POLR_AGG_SUM) {
			POLR_AP_REFUSE(POLR_E_UNSUPPORTED, "aggregate %u: a fused sink computes COUNT(*), COUNT and SUM", a);
		}
		if (const int rc = polr_agg_arg_rule(g, a, &pl->agg[a], err)) {
			return rc;
		}
		if (g.fn == POLR_AGG_SUM && g.col[0].width > 4) {
			// (the cells hold plain 64-bit sums: exact for 2^32 rows of values below 2^31)
			POLR_AP_REFUSE(POLR_E_UNSUPPORTED, "aggregate %u: a fused SUM takes columns of at most 4 bytes", a);
		}
	}
	return POLR_OK;
}

// The hashed sink's single allocation, as byte offsets: the table -- state, nulls, the counter block, keys, representative
// string cells (strings only), group cells -- and behind it the compacted groups: keys, representative cells, nulls, group
// cells.  The compacted keys and nulls are rounded up to 16 bytes, so that the uint4 cells and the group cells behind them
// stay aligned.  zero_bytes: the prefix (state, nulls, counters) that is zeroed before a run.
struct PolrHashAggLayout {
	uint64_t state, nulls, counters, keys, reps, cells, okeys, oreps, onulls, ocells;
	uint64_t zero_bytes, total;
};
static inline void polr_hashagg_layout(uint64_t capacity, uint64_t max_groups, uint32_t n_cols, uint32_t n_aggs, bool strings,
                                       uint64_t cell_bytes, uint64_t counter_bytes, PolrHashAggLayout *lo) {
	const uint64_t rep_bytes = strings ? 16 : 0;
	uint64_t at = 0;
	const auto take = [&at](uint64_t bytes) {
		const uint64_t off = at;
		at += bytes;
		return off;
	};
	lo->state = take(capacity * 4);
	lo->nulls = take(capacity * 4);
	lo->counters = take(counter_bytes);
	lo->zero_bytes = at;
	lo->keys = take(capacity * n_cols * 8);
	lo->reps = take(capacity * n_cols * rep_bytes);
	lo->cells = take(capacity * n_aggs * cell_bytes);
	lo->okeys = take((max_groups * n_cols * 8 + 15) & ~(uint64_t)15);
	lo->oreps = take(max_groups * n_cols * rep_bytes);
	lo->onulls = take((max_groups * 4 + 15) & ~(uint64_t)15);
	lo->ocells = take(max_groups * n_aggs * cell_bytes);
	lo->total = at;
}

// what the C ABI reports for an aggregate: COUNT is never NULL; the others are NULL when no row took part
static inline polr_agg_value polr_agg_decode(uint32_t fn, __int128 sum, long long mn, long long mx, unsigned long long count) {
	polr_agg_value v;
	memset(&v, 0, sizeof(v));
	v.count = count;
	switch (fn) {
	case POLR_AGG_COUNT_STAR:
	case POLR_AGG_COUNT:
		v.lo = (int64_t)count;
		break;
	case POLR_AGG_SUM:
		v.is_null = count == 0;
		v.lo = (int64_t)(unsigned long long)sum;
		v.hi = (int64_t)(sum >> 64);
		break;
	case POLR_AGG_MIN:
		v.is_null = count == 0;
		v.lo = count ? mn : 0;
		v.hi = (count && mn < 0) ? -1 : 0;
		break;
	default:
		v.is_null = count == 0;
		v.lo = count ? mx : 0;
		v.hi = (count && mx < 0) ? -1 : 0;
		break;
	}
	return v;
}
