// duckdb-polr_amd/csrc/polr_fuseagg_plan.h -- the fused UNGROUPED aggregate sink of the generic pool kernel
// (polr_out_fuse_aggregate / polr_out_fused_aggregate_result, include/polr_hip.h), as plain host code.  No HIP in here:
// polr_agg.hip describes the output and the columns (PolrAggArg, polr_agg_plan.h), allocates what the plan says and launches;
// the kernels (polr_gen_device.h: the fold; polr_agg.hip: fill and combine) take the word positions and kinds from the macros
// below; a stand-alone host program drives the header alone (tests/fuseagg/fuseagg_plan_main.cpp).
//
// The plan:
//   * every refusal of polr_out_fuse_aggregate, in this order, each with its message:
//       1. NULL output                                              POLR_E_INVALID
//          (specs == NULL or n_aggs == 0: un-fuse, never refused)
//       2. more than POLR_MAX_AGGS aggregates                       POLR_E_UNSUPPORTED
//       3. the output carries a fused sink already (either kind)    POLR_E_INVALID
//       4. per aggregate, in order -- the rule of polr_out_aggregate itself (polr_agg_arg_rule, polr_agg_plan.h):
//            an unknown function                                    POLR_E_INVALID
//            a column out of range                                  POLR_E_INVALID
//            a VARCHAR or unsigned 8-byte column                    POLR_E_UNSUPPORTED
//   * the cells: POLR_FUSEAGG_TABLES tables (a workgroup folds into table  blockIdx.x % tables) and one more behind them
//     where the read-out combines them; a table is 1 + 3 n_aggs 64-bit words:
//       word 0            the tuples folded (COUNT(*), and the bound of the SUM cells)
//       word 1 + 3a       aggregate a, SUM: the sum of (v & 0xFFFFFFFF);  MIN / MAX: the extreme of v ^ 2^63 as unsigned
//       word 2 + 3a       aggregate a, SUM: the sum of (v >> 32), arithmetic
//       word 3 + 3a       aggregate a: the rows that took part (non-NULL arguments)
//     every word is combined by ADD but the MIN word (unsigned min, "no rows" = all ones) and the MAX word (unsigned max,
//     "no rows" = 0): polr_fuseagg_word_kind / polr_fuseagg_reset_value;
//   * the decode of a combined table into polr_agg_value (polr_fuseagg_decode; the value itself: polr_agg_decode,
//     polr_agg_plan.h): the SUM is hi * 2^32 + lo in 128 bits --
//     exact while fewer than 2^32 tuples were folded (lo < 2^64, |hi| < 2^63); at 2^32 or more with a SUM in the sink the
//     call is POLR_E_RANGE and writes nothing.
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/polr_hip.h"
#include "polr_agg_plan.h"

#define POLR_FUSEAGG_MAX_AGGS POLR_AGG_MAX_AGGS // (= POLR_MAX_AGGS of polr_device.h: static_assert there)
#define POLR_FUSEAGG_TABLES 256u     // cell tables a launch's workgroups spread over
#define POLR_FUSEAGG_WORDS_PER_AGG 3u
#define POLR_FUSEAGG_MAX_WORDS (1u + POLR_FUSEAGG_WORDS_PER_AGG * POLR_FUSEAGG_MAX_AGGS)
#define POLR_FUSEAGG_ROWS 0u                    // word of the folded tuples
#define POLR_FUSEAGG_A(a) (1u + 3u * (a))       // SUM: low parts; MIN / MAX: the extreme in unsigned order
#define POLR_FUSEAGG_B(a) (2u + 3u * (a))       // SUM: high parts
#define POLR_FUSEAGG_N(a) (3u + 3u * (a))       // rows that took part
#define POLR_FUSEAGG_SIGN (1ull << 63)          // v ^ SIGN: signed order as unsigned order
#define POLR_FUSEAGG_ROW_LIMIT (1ull << 32)     // folded tuples below which the SUM cells are exact
enum { POLR_FUSEAGG_ADD = 0, POLR_FUSEAGG_MIN = 1, POLR_FUSEAGG_MAX = 2 };

// the sinks' request (polr_agg_plan.h); read here: has_out, has_specs, n_aggs, already_fused, and args[n_aggs] -- the column
// form, and only when the count is in range
typedef PolrAggRequest PolrFuseAggRequest;
struct PolrFuseAggPlan {
	char err[256];
	bool unfuse;
	uint32_t n_aggs;
	uint32_t fn[POLR_FUSEAGG_MAX_AGGS];
	PolrAggArgPlan agg[POLR_FUSEAGG_MAX_AGGS]; // the aggregates as the argument rule accepted them
	uint32_t n_tables, words_per_table;
	uint64_t cell_words;                      // of the allocation: (n_tables + 1) tables
	uint8_t kind[POLR_FUSEAGG_MAX_WORDS];     // POLR_FUSEAGG_ADD / _MIN / _MAX per word
	uint64_t reset[POLR_FUSEAGG_MAX_WORDS];   // what polr_out_reset writes into every table
	bool has_sum;
};

static inline uint32_t polr_fuseagg_word_kind(uint32_t fn, uint32_t word_of_agg) {
	if (word_of_agg == 0u && fn == POLR_AGG_MIN) {
		return POLR_FUSEAGG_MIN;
	}
	if (word_of_agg == 0u && fn == POLR_AGG_MAX) {
		return POLR_FUSEAGG_MAX;
	}
	return POLR_FUSEAGG_ADD;
}
static inline uint64_t polr_fuseagg_reset_value(uint32_t kind) {
	return kind == POLR_FUSEAGG_MIN ? ~0ull : 0ull;
}

#define POLR_FA_REFUSE(code_, ...)                                                                                     \
	do {                                                                                                               \
		snprintf(pl->err, sizeof(pl->err), __VA_ARGS__);                                                               \
		return (code_);                                                                                                \
	} while (0)

// POLR_OK with the plan filled (pl->unfuse: detach, nothing else is set), or the first refusal with pl->err
static inline int polr_fuseagg_plan(const PolrFuseAggRequest &rq, PolrFuseAggPlan *pl) {
	memset(pl, 0, sizeof(*pl));
	if (!rq.has_out) {
		POLR_FA_REFUSE(POLR_E_INVALID, "polr_out_fuse_aggregate: the output is NULL");
	}
	if (!rq.has_specs || rq.n_aggs == 0) {
		pl->unfuse = true;
		return POLR_OK;
	}
	if (rq.n_aggs > POLR_FUSEAGG_MAX_AGGS) {
		POLR_FA_REFUSE(POLR_E_UNSUPPORTED, "at most %u aggregates per call", POLR_FUSEAGG_MAX_AGGS);
	}
	if (rq.already_fused) {
		POLR_FA_REFUSE(POLR_E_INVALID, "the output object already has a fused sink");
	}
	pl->n_aggs = rq.n_aggs;
	pl->n_tables = POLR_FUSEAGG_TABLES;
	pl->words_per_table = 1u + POLR_FUSEAGG_WORDS_PER_AGG * rq.n_aggs;
	pl->cell_words = (uint64_t)(pl->n_tables + 1u) * pl->words_per_table;
	for (uint32_t a = 0; a < rq.n_aggs; a++) {
		const PolrAggArg &g = rq.args[a];
		if (const int rc = polr_agg_arg_rule(g, a, &pl->agg[a], pl->err)) {
			return rc;
		}
		pl->fn[a] = g.fn;
		pl->has_sum = pl->has_sum || g.fn == POLR_AGG_SUM;
		for (uint32_t w = 0; w < POLR_FUSEAGG_WORDS_PER_AGG; w++) {
			pl->kind[POLR_FUSEAGG_A(a) + w] = (uint8_t)polr_fuseagg_word_kind(g.fn, w);
		}
	}
	for (uint32_t w = 0; w < pl->words_per_table; w++) {
		pl->reset[w] = polr_fuseagg_reset_value(pl->kind[w]);
	}
	return POLR_OK;
}

// the combined table -> results[n_aggs].  POLR_E_RANGE (results untouched, err set) when the SUM cells may have wrapped.
static inline int polr_fuseagg_decode(const uint32_t *fn, uint32_t n_aggs, const uint64_t *cells, polr_agg_value *results,
                                      char *err, size_t err_len) {
	const uint64_t rows = cells[POLR_FUSEAGG_ROWS];
	for (uint32_t a = 0; a < n_aggs; a++) {
		if (fn[a] == POLR_AGG_SUM && rows >= POLR_FUSEAGG_ROW_LIMIT) {
			snprintf(err, err_len,
			         "aggregate %u: %llu tuples were folded since the last polr_out_reset; the cells of a fused SUM are exact "
			         "below 2^32; no result was written",
			         a, (unsigned long long)rows);
			return POLR_E_RANGE;
		}
	}
	for (uint32_t a = 0; a < n_aggs; a++) {
		const uint64_t n = fn[a] == POLR_AGG_COUNT_STAR ? rows : cells[POLR_FUSEAGG_N(a)];
		const __int128 sum = (__int128)(int64_t)cells[POLR_FUSEAGG_B(a)] * ((__int128)1 << 32) +
		                     (__int128)(unsigned __int128)cells[POLR_FUSEAGG_A(a)]; // (read for a SUM)
		const int64_t x = (int64_t)(cells[POLR_FUSEAGG_A(a)] ^ POLR_FUSEAGG_SIGN);     // (read for MIN, MAX)
		results[a] = polr_agg_decode(fn[a], sum, x, x, n);
	}
	return POLR_OK;
}
