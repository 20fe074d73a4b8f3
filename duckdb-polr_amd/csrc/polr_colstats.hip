// duckdb-polr_amd/csrc/polr_colstats.hip -- polr_ht_column_stats, polr_pipeline_column_stats, polr_ht_finalize_auto_stats:
// min / max / counts of columns that live on the device, in one pass (the NumericStatistics the reference's planner hands
// to PerfectHashJoinStats, plan_comparison_join.cpp:63-133).  Contract: include/polr_hip.h; the request checked and laid
// out: polr_colstats_plan.h.
//
// Two launches per call, whatever the number of columns:
//   partials    grid {workgroups, columns}: workgroup x of column y takes the tiles x, x + grid, ... of that column.  A lane
//               issues POLR_COLSTATS_LOADS 16-byte loads of cells together -- 16, 8, 4 or 2 cells each; of a VARCHAR cell only
//               the length word -- with the validity bytes of the same rows beside them (16, 8, 4, 2 or 1 bytes, one load),
//               and folds min, max, the valid count and the two VARCHAR sums in registers; then across the wave (shuffles),
//               across the four waves (LDS), and ONE record per workgroup goes out with plain stores.  A column's base is only
//               as aligned as its cells, its validity array not at all: the rows in front of the first 16-byte boundary of the
//               cells and behind the last whole load are read one by one (workgroup 0 of the column), the validity bytes
//               beside a load are read with whatever the address allows.  Through a selection list (the pipeline call with
//               POLR_STATS_SELECTED) a load is one row: the list is read coalesced, the cells where it points.
//   combine     one workgroup per column folds that column's records the same way and writes the record the host reads.
// No atomics anywhere; the results are exact integers, so the order of the folds cannot change them.  min and max are
// compared in ONE order for every type: the sign- or zero-extended value with its sign bit flipped if the column is signed,
// as uint64 (polr_colstats_finish turns it back).
// Every access is global_load / global_store: no FLAT instruction, no scratch.
// Algorithmic bytes per row and column: the cell width (4 for a VARCHAR cell: its length word; the 64-byte lines hold four
// cells) plus one validity byte if the column has an array; 4 more through a selection list.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "polr_colstats_plan.h"
#include "polr_internal.h"

// What ships is POLR_COLSTATS_SHAPE 0.  The other two are measurement builds (tools/bench_col_stats.py --ab, `make colstats-ab`),
// each in a small library of its own:
//   1   the shape of polr_key_minmax_kernel: one row per lane, a wave reduction, and per wave one atomic min, one atomic max
//       and the atomic adds of the counts on the column's ONE record; one launch for all columns
//   2   the shipped kernels, but the two launches once per column instead of once per call
#ifndef POLR_COLSTATS_SHAPE
#define POLR_COLSTATS_SHAPE 0
#endif

#define CS_U POLR_COLSTATS_LOADS
#define CS_BLOCK POLR_COLSTATS_BLOCK
#define CS_WORDS POLR_COLSTATS_WORDS

struct CsCol { // one column of a call (PolrColStatsShape with the column's addresses)
	const uint8_t *data, *valid;
	uint64_t head_rows, n_loads, tail_rows, n_tiles;
	uint32_t width, sx;
};
struct CsSet {
	CsCol c[POLR_MAX_STATS_COLS];
};

struct CsAcc {
	uint64_t mn, mx, n_valid, n_long, long_bytes;
};

// one cell folded in: v the cell's bits in the low `width` bytes (a VARCHAR cell: its length)
template <uint32_t W>
__device__ __forceinline__ void cs_take(CsAcc &a, uint64_t v, bool valid, bool sx) {
	uint64_t key;
	if (W == 1) {
		key = sx ? (uint64_t)(int64_t)(int8_t)v : (uint64_t)(uint8_t)v;
	} else if (W == 2) {
		key = sx ? (uint64_t)(int64_t)(int16_t)v : (uint64_t)(uint16_t)v;
	} else if (W == 4 || W == 16) {
		key = sx ? (uint64_t)(int64_t)(int32_t)v : (uint64_t)(uint32_t)v;
	} else {
		key = v;
	}
	key ^= sx ? POLR_COLSTATS_SIGN : 0ull;
	a.mn = valid && key < a.mn ? key : a.mn;
	a.mx = valid && key > a.mx ? key : a.mx;
	a.n_valid += valid ? 1u : 0u;
	if (W == 16) {
		const bool is_long = valid && (uint32_t)v > 12u;
		a.n_long += is_long ? 1u : 0u;
		a.long_bytes += is_long ? (uint64_t)(uint32_t)v : 0ull;
	}
}

// the validity bytes of the V rows of one load, as bits of a word each 8 apart (V <= 8) or as four words (V == 16).  The
// array starts wherever the caller's memory does: the bytes are copied, the compiler picks the widest load it may
template <uint32_t V>
struct CsValid {
	uint32_t w[(V + 3) / 4];
};
template <uint32_t V>
__device__ __forceinline__ CsValid<V> cs_load_valid(const POLR_GLOBAL uint8_t *p) {
	CsValid<V> r;
	uint8_t b[((V + 3) / 4) * 4] = {};
#pragma unroll
	for (uint32_t i = 0; i < V; i++) {
		b[i] = p[i];
	}
#pragma unroll
	for (uint32_t i = 0; i < (V + 3) / 4; i++) {
		r.w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
	}
	return r;
}
template <uint32_t V>
__device__ __forceinline__ bool cs_valid_at(const CsValid<V> &v, uint32_t j) {
	return ((v.w[j >> 2] >> (8u * (j & 3u))) & 0xFFu) != 0;
}

// cell j of a 16-byte load of W-byte cells
template <uint32_t W>
__device__ __forceinline__ uint64_t cs_cell(const uint4 &q, uint32_t j) {
	const uint32_t w[4] = {q.x, q.y, q.z, q.w};
	if (W == 8) {
		return (uint64_t)w[2 * j] | ((uint64_t)w[2 * j + 1] << 32);
	}
	if (W == 4) {
		return w[j];
	}
	if (W == 2) {
		return (w[j >> 1] >> (16u * (j & 1u))) & 0xFFFFu;
	}
	return (w[j >> 2] >> (8u * (j & 3u))) & 0xFFu;
}

// one row, read on its own: the head, the tail, and every row that comes through a selection list
template <uint32_t W>
__device__ __forceinline__ uint64_t cs_load_row(const POLR_GLOBAL uint8_t *data, uint64_t row) {
	if (W == 1) {
		return data[row];
	} else if (W == 2) {
		return ((const POLR_GLOBAL uint16_t *)data)[row];
	} else if (W == 4) {
		return ((const POLR_GLOBAL uint32_t *)data)[row];
	} else if (W == 8) {
		return ((const POLR_GLOBAL uint64_t *)data)[row];
	}
	return ((const POLR_GLOBAL uint32_t *)data)[row * 4u]; // a VARCHAR cell: its length word
}

// the tiles of a column whose rows lie one after the other: whole 16-byte loads
template <uint32_t W>
__device__ __forceinline__ void cs_fold_dense(const CsCol &c, CsAcc &a) {
	constexpr uint32_t V = W == 16 ? 1u : POLR_COLSTATS_VEC_BYTES / W;
	const POLR_GLOBAL uint8_t *data = as_global(c.data) + c.head_rows * W; // (at a 16-byte boundary, V > 1)
	const POLR_GLOBAL uint8_t *valid = c.valid ? as_global(c.valid) + c.head_rows : nullptr;
	const bool sx = c.sx != 0;
	for (uint64_t tile = blockIdx.x; tile < c.n_tiles; tile += gridDim.x) {
		uint64_t at[CS_U];
		bool in[CS_U];
		uint4 q[CS_U];
		CsValid<V> vb[CS_U];
#pragma unroll
		for (uint32_t u = 0; u < CS_U; u++) {
			const uint64_t load = (tile * CS_U + u) * CS_BLOCK + threadIdx.x;
			in[u] = load < c.n_loads;
			at[u] = in[u] ? load : 0; // (the loads are not predicated: they stay inside the column -- n_loads > 0 here)
		}
#pragma unroll
		for (uint32_t u = 0; u < CS_U; u++) {
			if (W == 16) {
				q[u] = make_uint4(((const POLR_GLOBAL uint32_t *)data)[at[u] * 4u], 0, 0, 0);
			} else {
				q[u] = load_global_x4((const POLR_GLOBAL uint32_t *)(data + at[u] * POLR_COLSTATS_VEC_BYTES));
			}
		}
		if (valid) {
#pragma unroll
			for (uint32_t u = 0; u < CS_U; u++) {
				vb[u] = cs_load_valid<V>(valid + at[u] * V);
			}
		} else {
#pragma unroll
			for (uint32_t u = 0; u < CS_U; u++) {
#pragma unroll
				for (uint32_t i = 0; i < (V + 3) / 4; i++) {
					vb[u].w[i] = 0x01010101u;
				}
			}
		}
#pragma unroll
		for (uint32_t u = 0; u < CS_U; u++) {
#pragma unroll
			for (uint32_t j = 0; j < V; j++) {
				cs_take<W>(a, W == 16 ? (uint64_t)q[u].x : cs_cell<W>(q[u], j), in[u] && cs_valid_at<V>(vb[u], j), sx);
			}
		}
	}
	// the rows in front of the first whole load and behind the last: at most 2 x 15, one lane each
	if (blockIdx.x == 0 && threadIdx.x < 64) {
		const uint64_t n_edge = c.head_rows + c.tail_rows;
		if (threadIdx.x < n_edge) {
			const uint64_t row = threadIdx.x < c.head_rows ? threadIdx.x : c.head_rows + c.n_loads * V + (threadIdx.x - c.head_rows);
			const POLR_GLOBAL uint8_t *cv = as_global(c.valid);
			const bool ok = cv ? cv[row] != 0 : true;
			cs_take<W>(a, cs_load_row<W>(as_global(c.data), row), ok, sx);
		}
	}
}

// ... and of a column read through a selection list: n_loads rows, one per load
template <uint32_t W>
__device__ __forceinline__ void cs_fold_selected(const CsCol &c, const POLR_GLOBAL uint32_t *sel, CsAcc &a) {
	const POLR_GLOBAL uint8_t *data = as_global(c.data);
	const POLR_GLOBAL uint8_t *valid = as_global(c.valid);
	const bool sx = c.sx != 0;
	for (uint64_t tile = blockIdx.x; tile < c.n_tiles; tile += gridDim.x) {
		uint64_t row[CS_U], cell[CS_U];
		bool in[CS_U];
		uint8_t vb[CS_U];
#pragma unroll
		for (uint32_t u = 0; u < CS_U; u++) {
			const uint64_t i = (tile * CS_U + u) * CS_BLOCK + threadIdx.x;
			in[u] = i < c.n_loads;
			row[u] = sel[in[u] ? i : 0];
		}
#pragma unroll
		for (uint32_t u = 0; u < CS_U; u++) {
			cell[u] = cs_load_row<W>(data, row[u]);
		}
#pragma unroll
		for (uint32_t u = 0; u < CS_U; u++) {
			vb[u] = valid ? valid[row[u]] : (uint8_t)1;
		}
#pragma unroll
		for (uint32_t u = 0; u < CS_U; u++) {
			cs_take<W>(a, cell[u], in[u] && vb[u] != 0, sx);
		}
	}
}

// a lane's record folded across the workgroup; lane 0 of wave 0 holds the result
__device__ __forceinline__ void cs_fold_workgroup(CsAcc &a) {
	__shared__ uint64_t lds[CS_BLOCK / 64][CS_WORDS];
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) {
		const uint64_t mn = __shfl_xor((unsigned long long)a.mn, d, 64), mx = __shfl_xor((unsigned long long)a.mx, d, 64);
		a.mn = mn < a.mn ? mn : a.mn;
		a.mx = mx > a.mx ? mx : a.mx;
		a.n_valid += __shfl_xor((unsigned long long)a.n_valid, d, 64);
		a.n_long += __shfl_xor((unsigned long long)a.n_long, d, 64);
		a.long_bytes += __shfl_xor((unsigned long long)a.long_bytes, d, 64);
	}
	const uint32_t wave = threadIdx.x >> 6;
	if ((threadIdx.x & 63) == 0) {
		lds[wave][0] = a.mn;
		lds[wave][1] = a.mx;
		lds[wave][2] = a.n_valid;
		lds[wave][3] = a.n_long;
		lds[wave][4] = a.long_bytes;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		for (uint32_t w = 1; w < CS_BLOCK / 64; w++) {
			a.mn = lds[w][0] < a.mn ? lds[w][0] : a.mn;
			a.mx = lds[w][1] > a.mx ? lds[w][1] : a.mx;
			a.n_valid += lds[w][2];
			a.n_long += lds[w][3];
			a.long_bytes += lds[w][4];
		}
	}
}

__device__ __forceinline__ void cs_store(uint64_t *rec, const CsAcc &a) {
	POLR_GLOBAL uint64_t *r = as_global(rec);
	r[0] = a.mn;
	r[1] = a.mx;
	r[2] = a.n_valid;
	r[3] = a.n_long;
	r[4] = a.long_bytes;
}

// partials[gridDim.y][gridDim.x][CS_WORDS]; sel: the selection list of every column (NULL: the rows as they lie)
__global__ __launch_bounds__(CS_BLOCK) void polr_colstats_kernel(CsSet cs, const uint32_t *__restrict__ sel,
                                                                  uint64_t *__restrict__ partials) {
	const CsCol &c = cs.c[blockIdx.y];
	CsAcc a = {~0ull, 0ull, 0ull, 0ull, 0ull};
	if (sel) {
		const POLR_GLOBAL uint32_t *s = as_global(sel);
		switch (c.width) {
		case 1: cs_fold_selected<1>(c, s, a); break;
		case 2: cs_fold_selected<2>(c, s, a); break;
		case 4: cs_fold_selected<4>(c, s, a); break;
		case 8: cs_fold_selected<8>(c, s, a); break;
		default: cs_fold_selected<16>(c, s, a); break;
		}
	} else {
		switch (c.width) {
		case 1: cs_fold_dense<1>(c, a); break;
		case 2: cs_fold_dense<2>(c, a); break;
		case 4: cs_fold_dense<4>(c, a); break;
		case 8: cs_fold_dense<8>(c, a); break;
		default: cs_fold_dense<16>(c, a); break;
		}
	}
	cs_fold_workgroup(a);
	if (threadIdx.x == 0) {
		cs_store(partials + ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * CS_WORDS, a);
	}
}

// result[gridDim.x][CS_WORDS]: the n_partials records of every column folded into one
__global__ __launch_bounds__(CS_BLOCK) void polr_colstats_combine_kernel(const uint64_t *__restrict__ partials, uint32_t n_partials,
                                                                          uint64_t *__restrict__ result) {
	const POLR_GLOBAL uint64_t *p = as_global(partials) + (uint64_t)blockIdx.x * n_partials * CS_WORDS;
	CsAcc a = {~0ull, 0ull, 0ull, 0ull, 0ull};
	for (uint32_t i = threadIdx.x; i < n_partials; i += CS_BLOCK) {
		const POLR_GLOBAL uint64_t *r = p + (uint64_t)i * CS_WORDS;
		a.mn = r[0] < a.mn ? r[0] : a.mn;
		a.mx = r[1] > a.mx ? r[1] : a.mx;
		a.n_valid += r[2];
		a.n_long += r[3];
		a.long_bytes += r[4];
	}
	cs_fold_workgroup(a);
	if (threadIdx.x == 0) {
		cs_store(result + (uint64_t)blockIdx.x * CS_WORDS, a);
	}
}

#if POLR_COLSTATS_SHAPE == 1
// the measured alternative: result[gridDim.y][CS_WORDS], initialised by the host; sel: as above
__global__ __launch_bounds__(CS_BLOCK) void polr_colstats_simple_kernel(CsSet cs, const uint32_t *__restrict__ sel, uint64_t n_rows,
                                                                         unsigned long long *result) {
	const CsCol &c = cs.c[blockIdx.y];
	const uint64_t i = (uint64_t)blockIdx.x * CS_BLOCK + threadIdx.x;
	CsAcc a = {~0ull, 0ull, 0ull, 0ull, 0ull};
	if (i < n_rows) {
		const uint64_t row = sel ? as_global(sel)[i] : i;
		const POLR_GLOBAL uint8_t *cv = as_global(c.valid);
		const bool ok = cv ? cv[row] != 0 : true;
		const POLR_GLOBAL uint8_t *d = as_global(c.data);
		const bool sx = c.sx != 0;
		switch (c.width) {
		case 1: cs_take<1>(a, cs_load_row<1>(d, row), ok, sx); break;
		case 2: cs_take<2>(a, cs_load_row<2>(d, row), ok, sx); break;
		case 4: cs_take<4>(a, cs_load_row<4>(d, row), ok, sx); break;
		case 8: cs_take<8>(a, cs_load_row<8>(d, row), ok, sx); break;
		default: cs_take<16>(a, cs_load_row<16>(d, row), ok, sx); break;
		}
	}
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) {
		const uint64_t mn = __shfl_xor((unsigned long long)a.mn, d, 64), mx = __shfl_xor((unsigned long long)a.mx, d, 64);
		a.mn = mn < a.mn ? mn : a.mn;
		a.mx = mx > a.mx ? mx : a.mx;
		a.n_valid += __shfl_xor((unsigned long long)a.n_valid, d, 64);
		a.n_long += __shfl_xor((unsigned long long)a.n_long, d, 64);
		a.long_bytes += __shfl_xor((unsigned long long)a.long_bytes, d, 64);
	}
	if ((threadIdx.x & 63) == 0 && a.n_valid) {
		unsigned long long *r = result + (uint64_t)blockIdx.y * CS_WORDS;
		atomicMin(&r[0], (unsigned long long)a.mn);
		atomicMax(&r[1], (unsigned long long)a.mx);
		atomicAdd(&r[2], (unsigned long long)a.n_valid);
		if (a.n_long) {
			atomicAdd(&r[3], (unsigned long long)a.n_long);
			atomicAdd(&r[4], (unsigned long long)a.long_bytes);
		}
	}
}
#endif

// the pass both entry points share, once the plan has accepted the request: columns[i] is the i-th named column
static int colstats_run(polr_ctx *ctx, void *stream, const PolrColStatsRequest &rq, const PolrColStatsColumn *shapes,
                        const PolrColStatsPlan &plan, const OwnedCol *const *columns, const uint32_t *sel, polr_col_stats *stats) {
	const uint64_t n_rows = rq.n_rows;
	std::vector<uint64_t> h_rec((size_t)plan.n_cols * CS_WORDS, 0);
	if (plan.grid_x) {
		HIPCHK(ctx, hipSetDevice(ctx->device));
		hipStream_t st = polr_stream(ctx, stream);
		if (st != ctx->stream) {
			// (the columns were uploaded, gathered or compacted on the context's stream unless the caller ordered otherwise)
			HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
		}
#if POLR_COLSTATS_SHAPE == 1
		DevBuf<unsigned long long> result;
		HIPCHK(ctx, result.alloc((uint64_t)plan.n_cols * CS_WORDS));
		for (uint32_t i = 0; i < plan.n_cols; i++) {
			h_rec[(size_t)i * CS_WORDS] = ~0ull;
		}
		HIPCHK(ctx, hipMemcpyAsync(result, h_rec.data(), h_rec.size() * 8, hipMemcpyHostToDevice, st));
		CsSet cs;
		memset(&cs, 0, sizeof(cs));
		for (uint32_t i = 0; i < plan.n_cols; i++) {
			cs.c[i] = CsCol{columns[i]->data, columns[i]->valid, 0, 0, 0, 0, columns[i]->width, (columns[i]->flags & POLR_COL_SIGNED) ? 1u : 0u};
		}
		hipLaunchKernelGGL(polr_colstats_simple_kernel, dim3((uint32_t)((n_rows + CS_BLOCK - 1) / CS_BLOCK), plan.n_cols), dim3(CS_BLOCK), 0,
		                   st, cs, sel, n_rows, result.get());
		HIPCHK(ctx, hipGetLastError());
		HIPCHK(ctx, hipMemcpyAsync(h_rec.data(), result, h_rec.size() * 8, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
#elif POLR_COLSTATS_SHAPE == 2
		std::vector<DevBuf<uint8_t>> scratch(plan.n_cols);
		for (uint32_t i = 0; i < plan.n_cols; i++) {
			PolrColStatsRequest one = rq;
			one.cols = &rq.cols[i];
			one.n_cols = 1;
			PolrColStatsPlan pl;
			POLR_TRY_PLAN(ctx, pl, polr_colstats_plan(one, shapes, pl));
			HIPCHK(ctx, scratch[i].alloc(pl.scratch_bytes));
			uint64_t *partials = (uint64_t *)(scratch[i].get() + pl.partials_off);
			uint64_t *result = (uint64_t *)(scratch[i].get() + pl.result_off);
			const PolrColStatsShape &s = pl.shape[0];
			CsSet cs;
			memset(&cs, 0, sizeof(cs));
			cs.c[0] = CsCol{columns[i]->data, columns[i]->valid, s.head_rows, s.n_loads, s.tail_rows, s.n_tiles, columns[i]->width,
			                (columns[i]->flags & POLR_COL_SIGNED) ? 1u : 0u};
			hipLaunchKernelGGL(polr_colstats_kernel, dim3(pl.grid_x, 1), dim3(CS_BLOCK), 0, st, cs, sel, partials);
			hipLaunchKernelGGL(polr_colstats_combine_kernel, dim3(1), dim3(CS_BLOCK), 0, st, (const uint64_t *)partials, pl.grid_x, result);
			HIPCHK(ctx, hipGetLastError());
			HIPCHK(ctx, hipMemcpyAsync(&h_rec[(size_t)i * CS_WORDS], result, CS_WORDS * 8, hipMemcpyDeviceToHost, st));
		}
		HIPCHK(ctx, hipStreamSynchronize(st));
#else
		DevBuf<uint8_t> scratch;
		HIPCHK(ctx, scratch.alloc(plan.scratch_bytes));
		uint64_t *partials = (uint64_t *)(scratch.get() + plan.partials_off);
		uint64_t *result = (uint64_t *)(scratch.get() + plan.result_off);
		CsSet cs;
		memset(&cs, 0, sizeof(cs));
		for (uint32_t i = 0; i < plan.n_cols; i++) {
			const PolrColStatsShape &s = plan.shape[i];
			cs.c[i] = CsCol{columns[i]->data, columns[i]->valid, s.head_rows, s.n_loads, s.tail_rows, s.n_tiles, columns[i]->width,
			                (columns[i]->flags & POLR_COL_SIGNED) ? 1u : 0u};
		}
		hipLaunchKernelGGL(polr_colstats_kernel, dim3(plan.grid_x, plan.n_cols), dim3(CS_BLOCK), 0, st, cs, sel, partials);
		hipLaunchKernelGGL(polr_colstats_combine_kernel, dim3(plan.n_cols), dim3(CS_BLOCK), 0, st, (const uint64_t *)partials,
		                   plan.grid_x, result);
		HIPCHK(ctx, hipGetLastError());
		HIPCHK(ctx, hipMemcpyAsync(h_rec.data(), result, h_rec.size() * 8, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
#endif
	}
	for (uint32_t i = 0; i < plan.n_cols; i++) {
		polr_colstats_finish(plan.grid_x ? &h_rec[(size_t)i * CS_WORDS] : nullptr, n_rows, columns[i]->width, columns[i]->flags, stats[i]);
	}
	return POLR_OK;
}

static const OwnedCol &cs_ht_col(const polr_ht *ht, uint32_t c) {
	uint32_t idx;
	return polr_htfilter_col(c, ht->n_keys, idx) ? ht->keys[idx] : ht->payload[idx];
}

extern "C" int polr_ht_column_stats(polr_ht *ht, void *stream, const uint32_t *cols, uint32_t n_cols, polr_col_stats *stats) {
	POLR_ENTRY();
	if (!ht) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = ht->ctx;
	PolrColStatsRequest rq = {};
	rq.who = "polr_ht_column_stats";
	rq.has_handle = true;
	rq.has_cols = cols != nullptr;
	rq.has_stats = stats != nullptr;
	rq.is_table = true;
	rq.finalized = ht->kind != KIND_NONE;
	rq.n_keys = ht->n_keys;
	rq.n_columns = ht->n_keys + ht->n_payload;
	rq.n_rows = ht->n_rows_in;
	rq.cols = cols;
	rq.n_cols = n_cols;
	std::vector<PolrColStatsColumn> shapes(rq.n_columns);
	if (!rq.finalized) { // (a finalized table from polr_pht_upload or polr_ht_alloc_like has no such columns)
		for (uint32_t c = 0; c < rq.n_columns; c++) {
			const OwnedCol &col = cs_ht_col(ht, c);
			shapes[c] = PolrColStatsColumn{col.width, col.flags, (uint64_t)(uintptr_t)col.data};
		}
	}
	PolrColStatsPlan plan;
	POLR_TRY_PLAN(ctx, plan, polr_colstats_plan(rq, shapes.data(), plan));
	const OwnedCol *columns[POLR_MAX_STATS_COLS];
	for (uint32_t i = 0; i < n_cols; i++) {
		columns[i] = &cs_ht_col(ht, cols[i]);
	}
	return colstats_run(ctx, stream, rq, shapes.data(), plan, columns, nullptr, stats);
}

extern "C" int polr_pipeline_column_stats(polr_pipeline *p, void *stream, const uint32_t *cols, uint32_t n_cols, uint32_t flags,
                                          polr_col_stats *stats) {
	POLR_ENTRY();
	if (!p) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = p->ctx;
	PolrColStatsRequest rq = {};
	rq.who = "polr_pipeline_column_stats";
	rq.has_handle = true;
	rq.has_cols = cols != nullptr;
	rq.has_stats = stats != nullptr;
	rq.n_columns = p->n_probe_cols;
	rq.flags = flags;
	rq.selected = (flags & POLR_STATS_SELECTED) && p->sel_dev;
	rq.n_rows = rq.selected ? p->n_tuples : p->n_probe_rows;
	rq.cols = cols;
	rq.n_cols = n_cols;
	std::vector<PolrColStatsColumn> shapes(rq.n_columns);
	for (uint32_t c = 0; c < rq.n_columns; c++) {
		const OwnedCol &col = p->probe_cols[c];
		shapes[c] = PolrColStatsColumn{col.width, col.flags, (uint64_t)(uintptr_t)col.data};
	}
	PolrColStatsPlan plan;
	POLR_TRY_PLAN(ctx, plan, polr_colstats_plan(rq, shapes.data(), plan));
	const OwnedCol *columns[POLR_MAX_STATS_COLS];
	for (uint32_t i = 0; i < n_cols; i++) {
		columns[i] = &p->probe_cols[cols[i]];
	}
	return colstats_run(ctx, stream, rq, shapes.data(), plan, columns, rq.selected ? p->sel_dev : nullptr, stats);
}

extern "C" int polr_ht_finalize_auto_stats(polr_ht *ht, void *stream, uint32_t *kind_out, polr_col_stats *key_stats) {
	POLR_ENTRY();
	if (!ht) {
		return POLR_E_INVALID;
	}
	polr_col_stats st = polr_col_stats();
	// (a finalized table: no pass, the finalizer refuses it as polr_ht_finalize_auto does)
	const bool pass = ht->kind == KIND_NONE && polr_colstats_finalize_needs_pass(ht->n_keys, ht->key_flags, key_stats != nullptr);
	if (pass) {
		const uint32_t key0 = 0;
		POLR_TRY(polr_ht_column_stats(ht, stream, &key0, 1, &st));
		if (key_stats) {
			*key_stats = st;
		}
	}
	bool tries_perfect;
	int rc;
	if (polr_colstats_finalize(ht->n_keys, ht->key_flags, ht->n_rows_in, pass, st, &tries_perfect) == POLR_CSF_AUTO) {
		rc = polr_ht_finalize_auto(ht, st.min_value, st.max_value, stream, kind_out);
	} else {
		rc = polr_ht_finalize_hash(ht, stream);
		if (!rc && kind_out) {
			*kind_out = ht->kind;
		}
	}
	return rc;
}

extern "C" int polr_col_stats_plan_info(uint64_t n_rows, uint32_t width, polr_col_stats_plan *info) {
	if (!info || !polr_colstats_width_ok(width)) {
		return POLR_E_INVALID;
	}
	const uint32_t col = 0;
	PolrColStatsRequest rq = {};
	rq.who = "polr_col_stats_plan_info";
	rq.has_handle = rq.has_cols = rq.has_stats = true;
	rq.n_columns = 1;
	rq.n_rows = n_rows;
	rq.cols = &col;
	rq.n_cols = 1;
	const PolrColStatsColumn shape = {width, 0, 0};
	PolrColStatsPlan plan;
	if (const int rc = polr_colstats_plan(rq, &shape, plan)) {
		return rc;
	}
	info->cells_per_load = plan.shape[0].cells_per_load;
	info->loads_in_flight = POLR_COLSTATS_LOADS;
	info->tile_rows = plan.shape[0].tile_rows;
	info->n_workgroups = plan.grid_x;
	info->stride_rows = plan.shape[0].stride_rows;
	info->scratch_bytes = plan.scratch_bytes;
	return POLR_OK;
}
