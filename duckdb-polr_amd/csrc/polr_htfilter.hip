// duckdb-polr_amd/csrc/polr_htfilter.hip -- polr_ht_filter: the rows of an un-finalized build side filtered and compacted
// on the device, between the upload and polr_ht_encode_dictionary* / polr_ht_finalize_* (the filtered dimension scan in
// front of PhysicalHashJoin::Sink, physical_hash_join.cpp:217-286: a PhysicalFilter or the scan's TableFilterSet).
// Contract: include/polr_hip.h; the request checked and laid out: polr_htfilter_plan.h; the evaluator: polr_fx_device.h, the
// one the source scan runs.
//
// Two passes over tiles of 1024 rows and one read-back between them:
//   counting    one wave per tile, 64 rows a step: fx_row_true, the ballot stored as the pass-bit word, the tile's count.
//               polr_chunk_prefix_kernel<uint32_t> then gives every tile its first output row and the total, which the host
//               reads once: the table's new allocation is sized by it.
//   compaction  a workgroup of four waves per tile; a wave has four consecutive words of the tile, a lane one row of each --
//               four independent loads in flight per lane and column.  It evaluates nothing: a kept row's output position is
//               its tile's first output row plus its rank among the tile's set bits (the popcounts of the words before its
//               own, the lane's rank inside it).  It writes the row number into the row list and, per column, the cell (1, 2,
//               4, 8 or 16 bytes, the 16 as one dwordx4) and the validity byte when the column has an array; the cell of a
//               NULL row is zero and its source is not read.  A wave whose four words are empty ends at once.  The column
//               descriptors -- up to 66 -- lie in a device array read through the constant address space: scalar loads.
//               Every other access is global_load / global_store: no FLAT instruction, no scratch.
// Algorithmic bytes per table row: the widths of the distinct filter columns plus their validity bytes, once; 2 x 1/8 for
// the pass bit; per kept row 4 for the row list and, over all columns, 2 x (width + validity).
//
// All columns go in ONE launch (a workgroup per tile serves every column), not one launch per column: on the workload of
// tools/bench_ht_filter.py (30 M rows, four columns, 1/5 kept) a call took 0.716 ms with one launch against 0.752 ms with
// one per column, 1.780 against 1.816 ms behind a LIKE.  These reads stream: there is no L2 to compete for as among the
// gathers of polr_ht_from_output, which preferred slot by slot.  (profiles/README.md, "Filtered build sides".)
// gfx950, the code object's metadata: counting 49 VGPRs / 106 SGPRs / 14 336 bytes of LDS (the matcher's), compaction
// 68 VGPRs / 52 SGPRs / no LDS; no scratch and no spills in either.
//
// Everything the table will hold is allocated before the first kernel writes, and moved into the table at the point of
// success: a refused or failed call leaves the table, its columns and polr_device_bytes_live() exactly as they were.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "polr_fx_device.h"
#include "polr_htfilter_plan.h"
#include "polr_internal.h"

#define HTF_R 4u // words of a tile a wave of the compaction kernel serves: a lane has one row of each

typedef PolrHtFilterDesc HtfCol;
static_assert(POLR_HTFILTER_TILE_WORDS * 64u == POLR_HTFILTER_TILE && POLR_HTFILTER_TILE_WORDS == 4u * HTF_R,
              "a tile is 16 words: four waves of four words");

// the counting pass: pass_bits[n_tiles * 16] (rows behind the table's last: 0), tile_count[n_tiles]
__global__ __launch_bounds__(256) void polr_htfilter_count_kernel(DevFxProg px, uint64_t n_rows, uint64_t n_tiles,
                                                                  unsigned long long *__restrict__ pass_bits,
                                                                  uint32_t *__restrict__ tile_count) {
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
	for (uint64_t tile = wave; tile < n_tiles; tile += n_waves) {
		const uint64_t begin = tile * POLR_HTFILTER_TILE;
		uint32_t cnt = 0;
		for (uint32_t w = 0; w < POLR_HTFILTER_TILE_WORDS; w++) {
			const uint64_t row = begin + w * 64u + lane;
			const bool pass = row < n_rows && fx_row_true(px, row);
			const uint64_t m = __ballot(pass);
			cnt += (uint32_t)__popcll(m);
			if (lane == 0) {
				as_global(pass_bits)[tile * POLR_HTFILTER_TILE_WORDS + w] = m;
			}
		}
		if (lane == 0) {
			as_global(tile_count)[tile] = cnt;
		}
	}
}

// HTF_R rows of one column: the validity bytes first, then the cells of the valid rows, then the stores
template <class T>
__device__ __forceinline__ void htf_cells(const POLR_GLOBAL uint8_t *src_valid, const POLR_GLOBAL uint8_t *src, POLR_GLOBAL uint8_t *dst,
                                          POLR_GLOBAL uint8_t *dst_valid, const uint64_t (&row)[HTF_R], const bool (&live)[HTF_R],
                                          const uint64_t (&pos)[HTF_R]) {
	bool valid[HTF_R];
	T v[HTF_R];
#pragma unroll
	for (uint32_t r = 0; r < HTF_R; r++) {
		valid[r] = live[r] && (!src_valid || src_valid[row[r]] != 0);
	}
#pragma unroll
	for (uint32_t r = 0; r < HTF_R; r++) {
		v[r] = (T)0;
		if (valid[r]) {
			v[r] = ((const POLR_GLOBAL T *)src)[row[r]];
		}
	}
#pragma unroll
	for (uint32_t r = 0; r < HTF_R; r++) {
		if (live[r]) {
			((POLR_GLOBAL T *)dst)[pos[r]] = v[r];
			if (dst_valid) {
				dst_valid[pos[r]] = valid[r] ? 1 : 0;
			}
		}
	}
}

// the compaction pass: grid.x the tile; every column of cols[n_cols] and the row list
__global__ __launch_bounds__(256) void polr_htfilter_compact_kernel(const unsigned long long *__restrict__ pass_bits_,
                                                                    const uint64_t *__restrict__ tile_base_, uint64_t n_tiles,
                                                                    const HtfCol *__restrict__ cols_, uint32_t n_cols,
                                                                    uint32_t *__restrict__ rows_) {
	const uint64_t tile = blockIdx.x;
	if (tile >= n_tiles) {
		return;
	}
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t w0 = uni(threadIdx.x >> 6) * HTF_R; // the wave's first word inside the tile
	const POLR_GLOBAL unsigned long long *bits = as_global(pass_bits_) + tile * POLR_HTFILTER_TILE_WORDS;
	uint64_t m[HTF_R];
	uint64_t any = 0;
#pragma unroll
	for (uint32_t r = 0; r < HTF_R; r++) {
		m[r] = uni64(bits[w0 + r]);
		any |= m[r];
	}
	if (!any) {
		return;
	}
	uint64_t out = as_global(tile_base_)[tile];
	for (uint32_t w = 0; w < w0; w++) {
		out += (uint64_t)__popcll(uni64(bits[w]));
	}
	bool live[HTF_R];
	uint64_t row[HTF_R], pos[HTF_R];
#pragma unroll
	for (uint32_t r = 0; r < HTF_R; r++) {
		live[r] = ((m[r] >> lane) & 1ull) != 0;
		row[r] = tile * POLR_HTFILTER_TILE + (uint64_t)(w0 + r) * 64u + lane;
		pos[r] = out + lane_rank(m[r]);
		out += (uint64_t)__popcll(m[r]);
	}
	POLR_GLOBAL uint32_t *rows = as_global(rows_);
#pragma unroll
	for (uint32_t r = 0; r < HTF_R; r++) {
		if (live[r]) {
			rows[pos[r]] = (uint32_t)row[r];
		}
	}
	const POLR_CONST HtfCol *cols = (const POLR_CONST HtfCol *)cols_;
	for (uint32_t c = 0; c < n_cols; c++) {
		const POLR_CONST HtfCol *d = cols + c;
		const POLR_GLOBAL uint8_t *sv = as_global(d->src_valid);
		const POLR_GLOBAL uint8_t *sd = as_global(d->src_data);
		POLR_GLOBAL uint8_t *dd = as_global(d->dst_data);
		POLR_GLOBAL uint8_t *dv = as_global(d->dst_valid);
		switch (d->width) {
		case 1:
			htf_cells<uint8_t>(sv, sd, dd, dv, row, live, pos);
			break;
		case 2:
			htf_cells<uint16_t>(sv, sd, dd, dv, row, live, pos);
			break;
		case 4:
			htf_cells<uint32_t>(sv, sd, dd, dv, row, live, pos);
			break;
		case 8:
			htf_cells<uint64_t>(sv, sd, dd, dv, row, live, pos);
			break;
		default:
			htf_cells<polr_u32x4>(sv, sd, dd, dv, row, live, pos);
			break;
		}
	}
}

// (n_tiles > 0) -- behind polr_ht_filter and polr_ht_semi_filter (polr_htsemi.hip), which counts with a kernel of its own
void polr_launch_htfilter_compact(hipStream_t st, const unsigned long long *pass_bits, const uint64_t *tile_base, uint64_t n_tiles,
                                  const PolrHtFilterDesc *cols, uint32_t n_cols, uint32_t *rows) {
	hipLaunchKernelGGL(polr_htfilter_compact_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, pass_bits, tile_base, n_tiles, cols,
	                   n_cols, rows);
}

// the guard of a VARCHAR filter column whose cells were never rebased onto a device heap: its non-NULL cells longer than 12
// bytes -- their pointers are the host's.  Reads the validity byte and the length word of a cell, nothing else.
__global__ __launch_bounds__(256) void polr_htfilter_count_long_kernel(const uint8_t *__restrict__ cells_,
                                                                       const uint8_t *__restrict__ valid_, uint64_t n_rows,
                                                                       unsigned long long *__restrict__ n_long) {
	const POLR_GLOBAL uint8_t *cells = as_global(cells_);
	const POLR_GLOBAL uint8_t *valid = as_global(valid_);
	unsigned long long mine = 0;
	for (uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n_rows; row += (uint64_t)gridDim.x * blockDim.x) {
		if (valid && !valid[row]) {
			continue;
		}
		mine += *(const POLR_GLOBAL uint32_t *)(cells + row * 16u) > 12u ? 1u : 0u;
	}
	mine = wave_sum64(mine);
	if ((threadIdx.x & 63u) == 0 && mine) {
		atomicAdd(n_long, mine);
	}
}

static OwnedCol &htf_col(polr_ht *ht, uint32_t c) {
	uint32_t idx;
	return polr_htfilter_col(c, ht->n_keys, idx) ? ht->keys[idx] : ht->payload[idx];
}

extern "C" int polr_ht_filter(polr_ht *ht, void *stream, const polr_filter_node *nodes, uint32_t n_nodes,
                              const polr_filter_value *values, uint32_t n_values, uint64_t *n_kept) {
	POLR_ENTRY();
	if (!ht) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = ht->ctx;
	// refusals before anything is enqueued
	PolrHtFilterRequest rq = {};
	rq.has_ht = true;
	rq.finalized = ht->kind != KIND_NONE;
	rq.filtered = ht->filtered;
	rq.has_dict = !ht->dicts.empty();
	rq.dict_col = rq.has_dict ? ht->dicts[0].src_col : 0;
	rq.n_keys = ht->n_keys;
	rq.n_payload = ht->n_payload;
	rq.n_rows = ht->n_rows_in;
	rq.nodes = nodes;
	rq.n_nodes = n_nodes;
	rq.values = values;
	rq.n_values = n_values;
	const uint32_t n_cols = ht->n_keys + ht->n_payload;
	std::vector<PolrHtFilterColumn> shapes(n_cols);
	for (uint32_t c = 0; c < n_cols; c++) {
		const OwnedCol &col = htf_col(ht, c);
		shapes[c] = PolrHtFilterColumn{col.width, col.flags & POLR_COL_SIGNED, col.valid != nullptr, col.owned(), col.strings_rebased};
	}
	PolrHtFilterPlan plan;
	POLR_TRY_PLAN(ctx, plan, polr_htfilter_plan(rq, shapes.data(), plan));
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	if (st != ctx->stream) {
		// (the columns were uploaded, and rebased onto their heaps, on the context's stream)
		HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	}
	const uint64_t n = ht->n_rows_in;
	DevBuf<uint8_t> scratch, prog;
	HIPCHK(ctx, scratch.alloc(plan.scratch_bytes));
	uint64_t *total = (uint64_t *)(scratch.get() + plan.total_off);
	// the heaps: a column some leaf reads that the library uploaded and whose heap never came holds inline strings only
	for (uint32_t c : plan.guard) {
		if (!n) {
			break;
		}
		const OwnedCol &col = htf_col(ht, c);
		unsigned long long h_long = 0;
		HIPCHK(ctx, hipMemsetAsync(total, 0, 8, st));
		const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)ctx->n_cus * 8);
		hipLaunchKernelGGL(polr_htfilter_count_long_kernel, dim3(grid), dim3(256), 0, st, (const uint8_t *)col.data,
		                   (const uint8_t *)col.valid, n, (unsigned long long *)total);
		HIPCHK(ctx, hipMemcpyAsync(&h_long, total, 8, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		if (h_long) {
			POLR_FAIL(ctx, POLR_E_INVALID,
			          "filter column %u: %llu rows hold strings longer than 12 bytes, but the column's heap was never put on the "
			          "device (polr_ht_set_payload_heaps)",
			          c, h_long);
		}
	}
	// the counting pass, the tiles' first output rows, the total
	uint64_t kept = 0;
	unsigned long long *bits = (unsigned long long *)(scratch.get() + plan.bits_off);
	uint64_t *tile_base = (uint64_t *)(scratch.get() + plan.base_off);
	uint32_t *tile_count = (uint32_t *)(scratch.get() + plan.count_off);
	PolrFxBlob blob; // (staged until the read-back below has synchronised the stream)
	if (n) {
		polr_fx_blob_make(plan.fx, blob);
		HIPCHK(ctx, prog.alloc(blob.bytes.size()));
		HIPCHK(ctx, hipMemcpyAsync(prog, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice, st));
		DevFxProg px;
		polr_fx_prog_make(plan.fx, blob, prog.get(), [&](uint32_t c) -> const OwnedCol & { return htf_col(ht, c); }, px);
		const uint32_t grid = (uint32_t)std::min<uint64_t>((plan.n_tiles + 3) / 4, (uint64_t)ctx->n_cus * 8);
		hipLaunchKernelGGL(polr_htfilter_count_kernel, dim3(grid), dim3(256), 0, st, px, n, plan.n_tiles, bits, tile_count);
		polr_launch_chunk_prefix(st, (const uint32_t *)tile_count, (uint32_t)plan.n_tiles, tile_base, total);
		HIPCHK(ctx, hipMemcpyAsync(&kept, total, 8, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
	}
	// everything the table will hold, before the first kernel that writes into it
	PolrHtFilterLayout lo;
	polr_htfilter_layout(shapes.data(), n_cols, kept, lo);
	DevBuf<uint8_t> col_mem;
	DevBuf<DevCol> keys_dev;
	HIPCHK(ctx, col_mem.alloc(lo.table_bytes));
	HIPCHK(ctx, keys_dev.alloc(ht->n_keys));
	std::vector<HtfCol> h_desc(n_cols);
	std::vector<DevCol> h_keys(ht->n_keys);
	for (uint32_t c = 0; c < n_cols; c++) {
		const OwnedCol &col = htf_col(ht, c);
		HtfCol &d = h_desc[c];
		d.src_data = col.data;
		d.src_valid = col.valid;
		d.dst_data = col_mem.get() + lo.data_off[c];
		d.dst_valid = col.valid ? col_mem.get() + lo.valid_off[c] : nullptr;
		d.width = col.width;
		d.pad = 0;
		if (c < ht->n_keys) {
			h_keys[c].data = d.dst_data;
			h_keys[c].valid = d.dst_valid;
			h_keys[c].width = col.width;
			h_keys[c].flags = col.flags;
		}
	}
	HtfCol *desc = (HtfCol *)(col_mem.get() + lo.desc_off);
	uint32_t *rows = (uint32_t *)(col_mem.get() + lo.rows_off);
	HIPCHK(ctx, hipMemcpyAsync(keys_dev.get(), h_keys.data(), ht->n_keys * sizeof(DevCol), hipMemcpyHostToDevice, st));
	if (kept) {
		HIPCHK(ctx, hipMemcpyAsync(desc, h_desc.data(), n_cols * sizeof(HtfCol), hipMemcpyHostToDevice, st));
		polr_launch_htfilter_compact(st, bits, tile_base, plan.n_tiles, desc, n_cols, rows);
		HIPCHK(ctx, hipGetLastError());
	}
	HIPCHK(ctx, hipStreamSynchronize(st)); // (the table is complete; the staged arrays and the scratch are locals)
	// nothing can fail from here on: the table takes what was built and lets go of what it held
	uint64_t freed = ht->col_mem.bytes();
	for (uint32_t c = 0; c < n_cols; c++) {
		OwnedCol &col = htf_col(ht, c);
		freed += col.own_data.bytes() + col.own_valid.bytes();
		col.lib_cells = col.owned();
		col.own_data.reset();
		col.own_valid.reset();
		col.data = h_desc[c].dst_data;
		col.valid = h_desc[c].dst_valid;
	}
	ht->col_mem = std::move(col_mem); // (frees the allocation of a table made by polr_ht_from_output)
	ht->keys_dev = std::move(keys_dev);
	ht->device_bytes = ht->device_bytes - freed + ht->col_mem.bytes();
	ht->n_rows_in = kept;
	ht->filter_rows = rows;
	ht->filtered = true;
	if (n_kept) {
		*n_kept = kept;
	}
	return POLR_OK;
}

extern "C" int polr_ht_fetch_filter_rows(polr_ht *ht, void *stream, uint32_t *dst, uint64_t dst_rows) {
	POLR_ENTRY();
	if (!ht) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = ht->ctx;
	if (!ht->filtered) {
		POLR_FAIL(ctx, POLR_E_INVALID, "polr_ht_fetch_filter_rows: the table was never filtered (polr_ht_filter)");
	}
	const uint64_t n = ht->n_rows_in; // (the build rows: since the filter, the kept rows)
	if (dst_rows < n) {
		POLR_FAIL(ctx, POLR_E_OVERFLOW, "polr_ht_fetch_filter_rows: room for %llu rows, the table kept %llu", (unsigned long long)dst_rows,
		          (unsigned long long)n);
	}
	if (!dst && n) {
		POLR_FAIL(ctx, POLR_E_INVALID, "polr_ht_fetch_filter_rows: dst is NULL");
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	if (n) {
		HIPCHK(ctx, hipMemcpyAsync(dst, ht->filter_rows, n * 4, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
	}
	return POLR_OK;
}
