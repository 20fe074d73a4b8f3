// duckdb-polr_amd/csrc/polr_filter_plan.h -- a polr_pipeline_scan_filter_expr program checked and lowered, as plain host
// code.  No HIP in here: polr_scan.hip calls polr_filter_plan() with the widths and signedness of the probe columns and
// uploads what it returns; a stand-alone host program drives it alone (tests/filterplan/filter_plan_main.cpp) and with the
// matcher (tests/like/like_main.cpp).
//
// The lowered form (what the scan kernel reads):
//   * nodes[]: the postfix program, one word per node -- POLR_FX_* in bits 0-7; leaves: the leaf's index in bits 8-15, its
//     column slot in bits 16-23 and, in bit 24, "never NULL" (IS [NOT] NULL);
//   * cols[]: the distinct columns named, at most POLR_FX_MAX_COLS, each with its leaves as one run of leaves[] -- the
//     kernel loads a row's cell once per column and evaluates that run against it;
//   * leaves[]: kind, comparison, and the leaf's range of values[];
//   * values[]: one entry per value of the call, index for index: the integer constant, the VARCHAR constant as
//     polr_strcmp.h takes it (polr_str_const; the bytes beyond 12 at bytes[bytes_off + 12]) and, for a value some LIKE leaf
//     names, the pattern as polr_like.h takes it;
//   * bytes[]: the VARCHAR constants and patterns of the call, one after the other; segs[]: the patterns' segments.
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/polr_hip.h"
#include "polr_like.h"
#include "polr_strcmp.h"

#define POLR_FX_MAX_COLS 8u
#define POLR_FX_NEVER_NULL (1u << 24)

struct PolrFxCol {
	uint32_t col;                  // probe-table column
	uint32_t first_leaf, n_leaves; // leaves[first_leaf .. first_leaf + n_leaves)
	uint32_t needs_cell;           // some leaf reads the cell (not only IS [NOT] NULL)
};
struct PolrFxLeaf {
	uint32_t kind, op; // POLR_FX_CMP / _IN / _LIKE; POLR_CMP_*
	uint32_t first_value, n_values;
};
struct PolrFxValue {
	polr_str_const c;
	int64_t constant;
	uint32_t bytes_off, pad;
	polr_like_pat pat;
};
struct PolrFilterColumn { // what the plan needs to know of a probe column
	uint32_t width, is_signed;
};
struct PolrFilterPlan {
	char err[200];
	uint32_t n_nodes, n_cols, n_leaves;
	uint32_t nodes[POLR_MAX_FILTER_NODES];
	PolrFxCol cols[POLR_FX_MAX_COLS];
	PolrFxLeaf leaves[POLR_MAX_FILTER_NODES];
	std::vector<PolrFxValue> values;
	std::vector<polr_like_seg> segs;
	std::vector<uint8_t> bytes;
};

#define POLR_FX_REFUSE(code_, ...)                                                                                     \
	do {                                                                                                               \
		snprintf(pl.err, sizeof(pl.err), __VA_ARGS__);                                                                 \
		return (code_);                                                                                                \
	} while (0)

// cut values[v]'s bytes at every '%' (see polr_like.h); '\0' in a pattern: the caller has refused it
static inline void polr_filter_lower_pattern(PolrFilterPlan &pl, uint32_t v, uint32_t len) {
	PolrFxValue &d = pl.values[v];
	const uint8_t *s = pl.bytes.data() + d.bytes_off;
	d.pat.first_seg = (uint32_t)pl.segs.size();
	d.pat.flags = d.pat.min_len = 0;
	uint32_t n_pieces = 0, begin = 0;
	for (uint32_t i = 0; i <= len; i++) {
		if (i < len && s[i] != '%') {
			continue;
		}
		// piece [begin, i): the first one is anchored at the front, the last one at the back, an empty one anchors nothing
		const bool first = n_pieces == 0, last = i == len;
		if (i > begin || (first && last)) {
			pl.segs.push_back(polr_like_seg{d.bytes_off + begin, i - begin});
			d.pat.flags |= (first ? POLR_LIKE_FRONT : 0u) | (last ? POLR_LIKE_BACK : 0u);
			d.pat.min_len += i - begin;
		}
		n_pieces++;
		begin = i + 1;
	}
	d.pat.n_segs = (uint32_t)pl.segs.size() - d.pat.first_seg;
}

// -> POLR_OK, or POLR_E_INVALID / POLR_E_UNSUPPORTED with pl.err set.  cols[n_cols]: the probe table's columns.
static inline int polr_filter_plan(const polr_filter_node *nodes, uint32_t n_nodes, const polr_filter_value *values,
                                   uint32_t n_values, const PolrFilterColumn *cols, uint32_t n_cols, PolrFilterPlan &pl) {
	pl.err[0] = 0;
	pl.n_nodes = pl.n_cols = pl.n_leaves = 0;
	pl.values.clear();
	pl.segs.clear();
	pl.bytes.clear();
	if ((!nodes && n_nodes) || (!values && n_values)) {
		POLR_FX_REFUSE(POLR_E_INVALID, "a count without its array");
	}
	if (n_nodes > POLR_MAX_FILTER_NODES) {
		POLR_FX_REFUSE(POLR_E_UNSUPPORTED, "an expression of %u nodes (at most %d)", n_nodes, POLR_MAX_FILTER_NODES);
	}
	if (n_values > POLR_MAX_FILTER_VALUES) {
		POLR_FX_REFUSE(POLR_E_UNSUPPORTED, "%u constants (at most %d)", n_values, POLR_MAX_FILTER_VALUES);
	}
	// the values: their bytes packed, the comparison form of each
	uint64_t total = 0;
	for (uint32_t v = 0; v < n_values; v++) {
		if (!values[v].str && values[v].str_len) {
			POLR_FX_REFUSE(POLR_E_INVALID, "value %u: a string constant of %llu bytes without its bytes", v,
			               (unsigned long long)values[v].str_len);
		}
		if (values[v].str_len > POLR_MAX_FILTER_STRING) {
			POLR_FX_REFUSE(POLR_E_UNSUPPORTED, "value %u: a string constant of %llu bytes (at most %d)", v,
			               (unsigned long long)values[v].str_len, POLR_MAX_FILTER_STRING);
		}
		total += values[v].str_len;
	}
	if (total > POLR_MAX_FILTER_BYTES) {
		POLR_FX_REFUSE(POLR_E_UNSUPPORTED, "%llu bytes of string constants (at most %d)", (unsigned long long)total,
		               POLR_MAX_FILTER_BYTES);
	}
	pl.values.resize(n_values);
	for (uint32_t v = 0; v < n_values; v++) {
		PolrFxValue &d = pl.values[v];
		memset(&d, 0, sizeof(d));
		d.constant = values[v].constant;
		d.bytes_off = (uint32_t)pl.bytes.size();
		d.c = polr_str_const_make((const uint8_t *)values[v].str, values[v].str_len);
		if (values[v].str_len) {
			pl.bytes.insert(pl.bytes.end(), (const uint8_t *)values[v].str, (const uint8_t *)values[v].str + values[v].str_len);
		}
	}
	// the nodes: every leaf against its column, the operand stack, the distinct columns
	uint32_t depth = 0, n_leaves = 0;
	uint32_t slot_of[POLR_MAX_FILTER_NODES], leaf_node[POLR_MAX_FILTER_NODES];
	for (uint32_t i = 0; i < n_nodes; i++) {
		const polr_filter_node &n = nodes[i];
		if (n.kind > POLR_FX_OR) {
			POLR_FX_REFUSE(POLR_E_INVALID, "node %u: unknown kind %u", i, n.kind);
		}
		if (n.kind == POLR_FX_NOT) {
			if (depth < 1) {
				POLR_FX_REFUSE(POLR_E_INVALID, "node %u: NOT on an empty stack", i);
			}
			continue;
		}
		if (n.kind == POLR_FX_AND || n.kind == POLR_FX_OR) {
			if (depth < 2) {
				POLR_FX_REFUSE(POLR_E_INVALID, "node %u: AND / OR needs two operands, the stack holds %u", i, depth);
			}
			depth--;
			continue;
		}
		if (n.col >= n_cols) {
			POLR_FX_REFUSE(POLR_E_INVALID, "node %u: column %u out of range", i, n.col);
		}
		const PolrFilterColumn &c = cols[n.col];
		const bool null_test = n.kind == POLR_FX_CMP && (n.op == POLR_CMP_IS_NULL || n.op == POLR_CMP_IS_NOT_NULL);
		if (n.kind == POLR_FX_CMP && n.op > POLR_CMP_IS_NOT_NULL) {
			POLR_FX_REFUSE(POLR_E_INVALID, "node %u: unknown comparison %u", i, n.op);
		}
		if (n.kind == POLR_FX_CMP && n.n_values != (null_test ? 0u : 1u)) {
			POLR_FX_REFUSE(POLR_E_INVALID, "node %u: a comparison with %u values", i, n.n_values);
		}
		if (n.kind == POLR_FX_IN && n.n_values == 0) {
			POLR_FX_REFUSE(POLR_E_INVALID, "node %u: IN without members", i);
		}
		if (n.kind == POLR_FX_LIKE && n.n_values != 1) {
			POLR_FX_REFUSE(POLR_E_INVALID, "node %u: LIKE takes one pattern, not %u", i, n.n_values);
		}
		if (n.first_value > n_values || n.n_values > n_values - n.first_value) {
			POLR_FX_REFUSE(POLR_E_INVALID, "node %u: values %u .. +%u outside the %u of the call", i, n.first_value, n.n_values,
			               n_values);
		}
		if (n.kind == POLR_FX_LIKE && c.width != 16) {
			POLR_FX_REFUSE(POLR_E_INVALID, "node %u: LIKE on column %u, which is %u bytes wide", i, n.col, c.width);
		}
		for (uint32_t v = n.first_value; v < n.first_value + n.n_values; v++) {
			if (values[v].str && c.width != 16) {
				POLR_FX_REFUSE(POLR_E_INVALID, "node %u: a string constant against column %u, which is %u bytes wide", i, n.col,
				               c.width);
			}
			if (c.width != 16 && !c.is_signed && values[v].constant < 0) {
				POLR_FX_REFUSE(POLR_E_INVALID, "node %u: negative constant against an unsigned column", i);
			}
			if (n.kind == POLR_FX_LIKE && values[v].str_len && memchr(values[v].str, 0, values[v].str_len)) {
				POLR_FX_REFUSE(POLR_E_UNSUPPORTED, "node %u: a NUL byte in a LIKE pattern (the escape character of a LIKE without ESCAPE)", i);
			}
		}
		if (depth == POLR_MAX_FILTER_DEPTH) {
			POLR_FX_REFUSE(POLR_E_UNSUPPORTED, "node %u: the operand stack grows beyond %d", i, POLR_MAX_FILTER_DEPTH);
		}
		depth++;
		uint32_t g = 0;
		while (g < pl.n_cols && pl.cols[g].col != n.col) {
			g++;
		}
		if (g == pl.n_cols) {
			if (pl.n_cols == POLR_FX_MAX_COLS) {
				POLR_FX_REFUSE(POLR_E_UNSUPPORTED, "more than %u distinct columns", POLR_FX_MAX_COLS);
			}
			pl.cols[pl.n_cols++] = PolrFxCol{n.col, 0, 0, 0};
		}
		pl.cols[g].n_leaves++;
		pl.cols[g].needs_cell |= null_test ? 0u : 1u;
		slot_of[i] = g;
		leaf_node[n_leaves++] = i;
	}
	if (n_nodes && depth != 1) {
		POLR_FX_REFUSE(POLR_E_INVALID, "the expression leaves %u values, not one", depth);
	}
	// lowered: leaves grouped per column, in program order inside a column
	uint32_t leaf_of[POLR_MAX_FILTER_NODES];
	for (uint32_t g = 0, at = 0; g < pl.n_cols; g++) {
		pl.cols[g].first_leaf = at;
		for (uint32_t l = 0; l < n_leaves; l++) {
			const uint32_t i = leaf_node[l];
			if (slot_of[i] != g) {
				continue;
			}
			const polr_filter_node &n = nodes[i];
			pl.leaves[at] = PolrFxLeaf{n.kind, n.kind == POLR_FX_CMP ? n.op : (uint32_t)POLR_CMP_EQ, n.first_value, n.n_values};
			if (n.kind == POLR_FX_LIKE && pl.values[n.first_value].pat.n_segs == 0 && pl.values[n.first_value].pat.flags == 0 &&
			    pl.values[n.first_value].pat.min_len == 0) {
				polr_filter_lower_pattern(pl, n.first_value, (uint32_t)values[n.first_value].str_len);
			}
			leaf_of[i] = at++;
		}
	}
	pl.n_leaves = n_leaves;
	pl.n_nodes = n_nodes;
	for (uint32_t i = 0; i < n_nodes; i++) {
		const polr_filter_node &n = nodes[i];
		pl.nodes[i] = n.kind;
		if (n.kind <= POLR_FX_LIKE) {
			const bool null_test = n.kind == POLR_FX_CMP && n.op >= POLR_CMP_IS_NULL;
			pl.nodes[i] |= (leaf_of[i] << 8) | (slot_of[i] << 16) | (null_test ? POLR_FX_NEVER_NULL : 0u);
		}
	}
	return POLR_OK;
}
