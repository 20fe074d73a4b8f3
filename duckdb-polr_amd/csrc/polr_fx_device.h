// duckdb-polr_amd/csrc/polr_fx_device.h -- the evaluator of a filter expression (polr_filter_plan.h lowers it), defined
// once for the two kernels that run it: the counting pass of the source scan (polr_tscan_count_expr_kernel, polr_scan.hip)
// and the counting pass of a build side's filter (polr_htfilter_count_kernel, polr_htfilter.hip).  What the reference
// evaluates in a PhysicalFilter -- OR / NOT trees, IN lists, LIKE -- as a postfix program.  The program is wave-uniform: the
// nodes travel in the kernel argument, leaves / values / segments / constant bytes in one device buffer read at uniform
// addresses; only the evaluation of a leaf is per lane.  A row first evaluates the leaves column by column -- the cell of a
// column is loaded once, a NULL row's cell never -- into one bit per leaf and one NULL bit per column, then walks the nodes
// over an operand stack of two 32-bit words per lane (true bits, NULL bits; a NULL's true bit is 0).
//
// Host side: polr_fx_blob_make() lays the program buffer out (values | leaves | segments | bytes) and polr_fx_prog_make()
// fills the kernel argument for a buffer at a device address; the caller names the table's columns.
#pragma once

#include <stdint.h>
#include <string.h>

#include <vector>

#include "polr_device.h"
#include "polr_filter_plan.h"
#include "polr_like.h"
#include "polr_strcmp.h"

struct DevFxCol {
	const uint8_t *data;
	const uint8_t *valid;
	uint32_t width, is_signed;
	uint32_t first_leaf, n_leaves;
	uint32_t needs_cell, pad;
};
struct DevFxProg {
	DevFxCol col[POLR_FX_MAX_COLS];
	uint32_t nodes[POLR_MAX_FILTER_NODES];
	const PolrFxLeaf *leaves;
	const PolrFxValue *values;
	const polr_like_seg *segs;
	const uint8_t *bytes;
	uint32_t n_cols, n_nodes;
};

// ---- the program buffer ------------------------------------------------------------------------------------------------
struct PolrFxBlob { // values | leaves | segments | bytes (8 spare bytes behind: never empty)
	std::vector<uint8_t> bytes;
	size_t values_at, leaves_at, segs_at, bytes_at;
};

static inline void polr_fx_blob_make(const PolrFilterPlan &pl, PolrFxBlob &b) {
	b.values_at = 0;
	b.leaves_at = b.values_at + pl.values.size() * sizeof(PolrFxValue);
	b.segs_at = b.leaves_at + pl.n_leaves * sizeof(PolrFxLeaf);
	b.bytes_at = b.segs_at + pl.segs.size() * sizeof(polr_like_seg);
	b.bytes.assign(b.bytes_at + pl.bytes.size() + 8, 0);
	if (!pl.values.empty()) {
		memcpy(b.bytes.data() + b.values_at, pl.values.data(), pl.values.size() * sizeof(PolrFxValue));
	}
	memcpy(b.bytes.data() + b.leaves_at, pl.leaves, pl.n_leaves * sizeof(PolrFxLeaf));
	if (!pl.segs.empty()) {
		memcpy(b.bytes.data() + b.segs_at, pl.segs.data(), pl.segs.size() * sizeof(polr_like_seg));
	}
	if (!pl.bytes.empty()) {
		memcpy(b.bytes.data() + b.bytes_at, pl.bytes.data(), pl.bytes.size());
	}
}

// the kernel argument of a program whose buffer lies at `dev`; column(c) is table column c as the kernels read it: an
// object with data, valid, width and flags (OwnedCol)
template <class ColumnOf>
static inline void polr_fx_prog_make(const PolrFilterPlan &pl, const PolrFxBlob &b, const uint8_t *dev, ColumnOf column, DevFxProg &px) {
	memset(&px, 0, sizeof(px));
	px.n_cols = pl.n_cols;
	px.n_nodes = pl.n_nodes;
	memcpy(px.nodes, pl.nodes, sizeof(uint32_t) * pl.n_nodes);
	for (uint32_t g = 0; g < pl.n_cols; g++) {
		const auto &c = column(pl.cols[g].col);
		DevFxCol &d = px.col[g];
		d.data = c.data;
		d.valid = c.valid;
		d.width = c.width;
		d.is_signed = c.flags & 1u;
		d.first_leaf = pl.cols[g].first_leaf;
		d.n_leaves = pl.cols[g].n_leaves;
		d.needs_cell = pl.cols[g].needs_cell;
	}
	px.values = (const PolrFxValue *)(dev + b.values_at);
	px.leaves = (const PolrFxLeaf *)(dev + b.leaves_at);
	px.segs = (const polr_like_seg *)(dev + b.segs_at);
	px.bytes = dev + b.bytes_at;
}

#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
// value OP constant on integers: the six comparisons of a ConstantFilter, in the column's signedness
__device__ __forceinline__ bool int_cmp_holds(uint64_t v, int64_t constant, uint32_t op, bool is_signed) {
	if (is_signed) {
		const int64_t a = (int64_t)v, c = constant;
		return op == POLR_CMP_EQ   ? a == c
		       : op == POLR_CMP_NE ? a != c
		       : op == POLR_CMP_LT ? a < c
		       : op == POLR_CMP_GT ? a > c
		       : op == POLR_CMP_LE ? a <= c
		                           : a >= c;
	}
	const uint64_t c = (uint64_t)constant; // (host: constant >= 0 for unsigned columns)
	return op == POLR_CMP_EQ   ? v == c
	       : op == POLR_CMP_NE ? v != c
	       : op == POLR_CMP_LT ? v < c
	       : op == POLR_CMP_GT ? v > c
	       : op == POLR_CMP_LE ? v <= c
	                           : v >= c;
}

// does the integer v compare (op) with one of the leaf's constants?  (CMP: one constant; IN: op is EQ)
__device__ __forceinline__ bool fx_leaf_int(const DevFxProg &px, const PolrFxLeaf lf, uint64_t v, bool is_signed) {
	bool r = false;
	for (uint32_t i = lf.first_value; i < lf.first_value + lf.n_values; i++) {
		r = r || int_cmp_holds(v, px.values[i].constant, lf.op, is_signed);
	}
	return r;
}

__device__ __forceinline__ bool fx_leaf_str(const DevFxProg &px, const PolrFxLeaf lf, const uint4 cell) {
	if (lf.kind == POLR_FX_LIKE) {
		return polr_like_match(cell.x, cell.y, cell.z, cell.w, px.values[lf.first_value].pat, px.segs, px.bytes);
	}
	bool r = false;
	for (uint32_t i = lf.first_value; i < lf.first_value + lf.n_values && !r; i++) {
		const polr_str_const c = px.values[i].c;
		if (lf.op == POLR_CMP_EQ && c.len != cell.x) {
			continue; // (equal strings have equal lengths: most IN members end here)
		}
		r = polr_str_cmp_holds(polr_str_cmp3(cell.x, cell.y, cell.z, cell.w, c, px.bytes + px.values[i].bytes_off + 12u), lf.op);
	}
	return r;
}

// is the root TRUE for the row?
__device__ __forceinline__ bool fx_row_true(const DevFxProg &px, uint64_t row) {
	unsigned long long leaf_true = 0;
	uint32_t col_null = 0;
	for (uint32_t c = 0; c < px.n_cols; c++) {
		const DevFxCol &col = px.col[c];
		const bool valid = !(col.valid && !as_global(col.valid)[row]);
		col_null |= valid ? 0u : 1u << c;
		uint4 cell = make_uint4(0, 0, 0, 0);
		uint64_t v = 0;
		if (valid && col.needs_cell) {
			if (col.width == 16) {
				cell = load_global_x4(as_global((const uint32_t *)col.data) + row * 4);
			} else {
				v = load_cell(as_global(col.data) + row * col.width, col.width, col.is_signed != 0);
			}
		}
		for (uint32_t l = col.first_leaf; l < col.first_leaf + col.n_leaves; l++) {
			const PolrFxLeaf lf = px.leaves[l];
			bool t;
			if (lf.kind == POLR_FX_CMP && lf.op >= POLR_CMP_IS_NULL) {
				t = (lf.op == POLR_CMP_IS_NULL) != valid;
			} else if (!valid) {
				t = false; // NULL: the node takes the column's NULL bit
			} else if (col.width == 16) {
				t = fx_leaf_str(px, lf, cell);
			} else {
				t = fx_leaf_int(px, lf, v, col.is_signed != 0);
			}
			leaf_true |= (unsigned long long)t << l;
		}
	}
	uint32_t T = 0, N = 0; // the operand stack: bit 0 is the top
	for (uint32_t i = 0; i < px.n_nodes; i++) {
		const uint32_t nd = px.nodes[i];
		const uint32_t kind = nd & 0xFFu;
		if (kind <= POLR_FX_LIKE) {
			const uint32_t n = (nd & POLR_FX_NEVER_NULL) ? 0u : (col_null >> ((nd >> 16) & 0xFFu)) & 1u;
			const uint32_t t = (uint32_t)(leaf_true >> ((nd >> 8) & 0xFFu)) & 1u & ~n;
			T = (T << 1) | t;
			N = (N << 1) | n;
		} else if (kind == POLR_FX_NOT) {
			T ^= ~N & 1u; // NOT NULL = NULL
		} else {
			const uint32_t ta = (T >> 1) & 1u, tb = T & 1u, na = (N >> 1) & 1u, nb = N & 1u;
			uint32_t rt, rn;
			if (kind == POLR_FX_AND) {
				const uint32_t rf = (~(ta | na) | ~(tb | nb)) & 1u; // one side FALSE: FALSE, whatever the other is
				rt = ta & tb;
				rn = (na | nb) & ~rf;
			} else {
				rt = ta | tb; // one side TRUE: TRUE
				rn = (na | nb) & ~rt;
			}
			T = ((T >> 2) << 1) | rt;
			N = ((N >> 2) << 1) | rn;
		}
	}
	return px.n_nodes == 0 || (T & 1u);
}
#endif
