// duckdb-polr_amd/csrc/polr_strout.hip -- polr_out_materialize_strings: a VARCHAR column of the output as complete
// string_t cells plus a packed heap of the long strings' bytes, in the destination's address space (late materialisation
// of strings: RowOperations::Gather for string_t, row_gather.cpp:47-86).  Contract: include/polr_hip.h.
//
// Two passes over the output chunks, one workgroup per chunk as in the cell gather (polr_gather.hip):
//   measure  one lane per output row reads the row id, the validity byte and the 4-byte length word of the cell -- never
//            a pointer.  A workgroup scan gives every row its 64-bit byte offset inside its chunk (scratch: 8 bytes per
//            output row) and the chunk its byte total; long cells are counted on the way (the guard of a column whose heap
//            never came).  polr_launch_chunk_prefix turns the chunk totals into chunk offsets, 64-bit throughout, and the
//            host reads the grand total back ONCE: overflow and the guard are decided before anything is written.
//   write    one lane per output row loads the cell, stores the normalised cell with one 16-byte store (inline: padding
//            zeroed; long: the pointer into the destination heap; NULL: zeros, source cell not read), and copies the bytes
//            (polr_strcopy.h).  Work is divided by bytes: a string of up to `lane_max` bytes is copied by its own lane,
//            a longer one by the whole wave with lanes striding over its words, so a 1 MB string costs length / 512 steps
//            of one wave instead of length / 8 of one lane.
// Algorithmic bytes per output row: 4 (id) + 1 (validity) + 4 (length) read in the first pass; 4 + 1 + 16 read and 16 + 1
// written in the second; 8 written and read for the row offset; plus twice the heap bytes (read once, written once).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "polr_internal.h"
#include "polr_strcopy.h"

// the 64-bit inclusive prefix over the lanes of a wave
__device__ __forceinline__ uint64_t wave_inclusive_scan64(uint64_t v, uint32_t lane) {
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint64_t o = __shfl_up(v, d, 64);
		if ((int)lane >= d) {
			v += o;
		}
	}
	return v;
}

// row_off[chunk_base + i] = heap bytes of the rows of this chunk before row i; chunk_bytes[chunk] = those of the chunk
__global__ __launch_bounds__(256) void polr_strout_measure_kernel(DevOut out, const uint64_t *__restrict__ chunk_base_,
                                                                   uint32_t n_chunks, uint32_t slot, DevCol src,
                                                                   uint64_t *__restrict__ row_off_,
                                                                   uint64_t *__restrict__ chunk_bytes,
                                                                   unsigned long long *__restrict__ n_long) {
	__shared__ uint64_t wave_total[4];
	const uint32_t chunk = blockIdx.x;
	if (chunk >= n_chunks) {
		return;
	}
	const uint32_t n = as_global(out.chunk_count)[chunk];
	const POLR_GLOBAL uint32_t *ids = as_global(out.ids) + (uint64_t)slot * out.slot_stride + (uint64_t)chunk * out.chunk_capacity;
	const POLR_GLOBAL uint8_t *valid_col = as_global(src.valid);
	const POLR_GLOBAL uint8_t *cells = as_global(src.data);
	POLR_GLOBAL uint64_t *row_off = as_global(row_off_) + as_global(chunk_base_)[chunk];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
	uint64_t carry = 0, longs = 0;
	for (uint32_t start = 0; start < n; start += blockDim.x) { // (every wave takes every turn: the barriers below)
		const uint32_t i = start + threadIdx.x;
		uint64_t bytes = 0;
		if (i < n) {
			const uint32_t row = ids[i];
			if (!valid_col || valid_col[row]) {
				bytes = polr_str_heap_bytes(*(const POLR_GLOBAL uint32_t *)(cells + (uint64_t)row * 16u), true);
			}
		}
		longs += bytes ? 1u : 0u;
		const uint64_t incl = wave_inclusive_scan64(bytes, lane);
		if (lane == 63u) {
			wave_total[wave] = incl;
		}
		__syncthreads();
		uint64_t before = 0, all = 0;
		for (uint32_t w = 0; w < n_waves; w++) {
			const uint64_t t = wave_total[w];
			before += w < wave ? t : 0ull;
			all += t;
		}
		if (i < n) {
			row_off[i] = carry + before + incl - bytes;
		}
		carry += all;
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		as_global(chunk_bytes)[chunk] = carry;
	}
	longs = wave_sum64(longs);
	if (lane == 0 && longs) {
		atomicAdd(n_long, (unsigned long long)longs);
	}
}

// heap_dev: where the bytes are written; heap_addr: the address of the same heap in the destination's address space, which
// the cells carry (the two differ when the destination is host memory and the heap is staged)
__global__ __launch_bounds__(256) void polr_strout_write_kernel(DevOut out, const uint64_t *__restrict__ chunk_base_,
                                                                 uint32_t n_chunks, uint32_t slot, DevCol src,
                                                                 const uint64_t *__restrict__ row_off_,
                                                                 const uint64_t *__restrict__ chunk_heap_base,
                                                                 uint4 *__restrict__ dst_cells_, uint8_t *__restrict__ dst_valid_,
                                                                 uint8_t *heap_dev, uint64_t heap_addr, uint32_t lane_max) {
	const uint32_t chunk = blockIdx.x;
	if (chunk >= n_chunks) {
		return;
	}
	const uint32_t n = as_global(out.chunk_count)[chunk];
	const uint64_t base = as_global(chunk_base_)[chunk];
	const uint64_t heap_base = as_global(chunk_heap_base)[chunk];
	const POLR_GLOBAL uint32_t *ids = as_global(out.ids) + (uint64_t)slot * out.slot_stride + (uint64_t)chunk * out.chunk_capacity;
	const POLR_GLOBAL uint8_t *valid_col = as_global(src.valid);
	const POLR_GLOBAL uint32_t *cells = as_global((const uint32_t *)src.data);
	const POLR_GLOBAL uint64_t *row_off = as_global(row_off_) + base;
	POLR_GLOBAL polr_u32x4 *dst_cells = (POLR_GLOBAL polr_u32x4 *)as_global(dst_cells_) + base;
	POLR_GLOBAL uint8_t *dst_valid = dst_valid_ ? as_global(dst_valid_) + base : nullptr;
	const uint32_t lane = threadIdx.x & 63u;
	for (uint32_t start = (threadIdx.x & ~63u); start < n; start += blockDim.x) { // (start: the wave's first row)
		const uint32_t i = start + lane;
		uint32_t len = 0; // > 0: a long string, to be copied from s to d
		uint64_t s = 0, d = 0;
		if (i < n) {
			const uint32_t row = ids[i];
			const bool valid = !valid_col || valid_col[row];
			polr_u32x4 cell = {0u, 0u, 0u, 0u};
			if (valid) {
				const uint4 c = load_global_x4(cells + (uint64_t)row * 4u);
				if (c.x <= 12u) {
					cell.x = c.x;
					cell.y = c.y & polr_str_word_mask(c.x, 0);
					cell.z = c.z & polr_str_word_mask(c.x, 1);
					cell.w = c.w & polr_str_word_mask(c.x, 2);
				} else {
					const uint64_t off = heap_base + row_off[i];
					const uint64_t addr = heap_addr + off;
					cell.x = c.x;
					cell.y = c.y;
					cell.z = (uint32_t)addr;
					cell.w = (uint32_t)(addr >> 32);
					len = c.x;
					s = ((uint64_t)c.w << 32) | c.z;
					d = (uint64_t)heap_dev + off;
				}
			}
			dst_cells[i] = cell;
			if (dst_valid) {
				dst_valid[i] = valid ? 1 : 0;
			}
			if (len && len <= lane_max) {
				polr_str_copy((uint8_t *)d, (const uint8_t *)s, len, 0u, 1u);
			}
		}
		// the strings beyond the cut-over, one after the other, by the whole wave
		uint64_t wide = __ballot(len > lane_max);
		while (wide) {
			const int l = __ffsll((unsigned long long)wide) - 1;
			wide &= wide - 1;
			const uint64_t ws = __shfl(s, l, 64), wd = __shfl(d, l, 64);
			const uint32_t wlen = __shfl(len, l, 64);
			polr_str_copy((uint8_t *)wd, (const uint8_t *)ws, wlen, lane, 64u);
		}
	}
}

// workgroup size of both passes: a wave per 64 rows of a chunk's capacity, four at the most
uint32_t polr_strout_block(const polr_out *o) {
	return std::min<uint32_t>(256u, (o->dev.chunk_capacity + 63u) / 64u * 64u);
}

// the two passes over the chunks the output's statistics count (polr_out_materialize_strings below; polr_ht_from_output,
// polr_fromout.hip)
void polr_launch_strout_measure(hipStream_t st, const polr_out *o, uint32_t slot, DevCol src, uint64_t *row_off,
                                uint64_t *chunk_bytes, unsigned long long *n_long) {
	hipLaunchKernelGGL(polr_strout_measure_kernel, dim3(o->n_chunks), dim3(polr_strout_block(o)), 0, st, o->dev,
	                   o->chunk_base.get(), o->n_chunks, slot, src, row_off, chunk_bytes, n_long);
}

void polr_launch_strout_write(hipStream_t st, const polr_out *o, uint32_t slot, DevCol src, const uint64_t *row_off,
                              const uint64_t *chunk_heap_base, uint4 *dst_cells, uint8_t *dst_valid, uint8_t *heap_dev,
                              uint64_t heap_addr) {
	hipLaunchKernelGGL(polr_strout_write_kernel, dim3(o->n_chunks), dim3(polr_strout_block(o)), 0, st, o->dev,
	                   o->chunk_base.get(), o->n_chunks, slot, src, row_off, chunk_heap_base, dst_cells, dst_valid, heap_dev,
	                   heap_addr, (uint32_t)POLR_STRCOPY_LANE_MAX);
}

extern "C" int polr_out_materialize_strings(polr_out *o, void *stream, int32_t src_join, uint32_t src_col, void *dst_cells,
                                            uint8_t *dst_valid, uint64_t dst_rows, void *dst_heap, uint64_t heap_cap,
                                            uint64_t *heap_used, uint32_t dst_flags) {
	POLR_ENTRY();
	if (!o || !heap_used) {
		return POLR_E_INVALID;
	}
	*heap_used = 0;
	polr_pipeline *p = o->pipe;
	polr_ctx *ctx = p->ctx;
	// refusals, in this order, before anything is enqueued (the output's own statistics apart)
	if (o->fused_dev) {
		POLR_FAIL(ctx, POLR_E_INVALID, "the output has a fused GROUP BY sink: it holds group cells, no row ids to materialise");
	}
	POLR_REFUSE_AGG_CELLS(ctx, o);
	if (!dst_heap && heap_cap) {
		POLR_FAIL(ctx, POLR_E_INVALID, "a heap of %llu bytes at NULL", (unsigned long long)heap_cap);
	}
	OutCol c;
	POLR_TRY(polr_out_col(p, src_join, src_col, &c, "column", src_col));
	if (c.dev.width != 16) {
		POLR_FAIL(ctx, POLR_E_INVALID, "not a VARCHAR column (%u-byte cells)", c.dev.width);
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	POLR_TRY(out_ensure_stats(o, stream));
	const uint64_t n = o->n_rows;
	if (dst_rows < n) {
		POLR_FAIL(ctx, POLR_E_INVALID, "destination holds %llu rows, output has %llu", (unsigned long long)dst_rows,
		          (unsigned long long)n);
	}
	if (!dst_cells && n) {
		POLR_FAIL(ctx, POLR_E_INVALID, "no destination for the cells of %llu rows", (unsigned long long)n);
	}
	if (n == 0) {
		return POLR_OK; // (also an output no materialising run has filled: it has no rows)
	}
	// measure
	const uint32_t nc = o->n_chunks;
	DevBuf<uint64_t> row_off, chunk_words; // chunk_words: [nc] byte totals, [nc] their exclusive prefix, the total, the long cells
	HIPCHK(ctx, row_off.alloc(n));
	HIPCHK(ctx, chunk_words.alloc(2ull * nc + 2));
	uint64_t *chunk_bytes = chunk_words.get(), *chunk_heap_base = chunk_bytes + nc, *tail = chunk_heap_base + nc;
	HIPCHK(ctx, hipMemsetAsync(tail, 0, 16, st));
	polr_launch_strout_measure(st, o, c.slot, c.dev, row_off.get(), chunk_bytes, (unsigned long long *)(tail + 1));
	polr_launch_chunk_prefix(st, (const uint64_t *)chunk_bytes, nc, chunk_heap_base, tail);
	uint64_t h_tail[2] = {0, 0};
	HIPCHK(ctx, hipMemcpyAsync(h_tail, tail, 16, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	const uint64_t total = h_tail[0], n_long = h_tail[1];
	if (n_long && !c.col->strings_rebased && c.col->owned()) {
		// (the library's own upload, never rebased onto a device heap: the pointers of its long cells are the host's)
		POLR_FAIL_HEAP_NEVER_CAME(ctx, "column", src_col, n_long);
	}
	*heap_used = total;
	if (heap_cap < total) {
		POLR_FAIL(ctx, POLR_E_OVERFLOW, "the strings take %llu heap bytes, the destination holds %llu",
		          (unsigned long long)total, (unsigned long long)heap_cap);
	}
	// write
	const bool to_device = (dst_flags & POLR_COL_DEVICE) != 0;
	uint4 *d_cells = (uint4 *)dst_cells;
	uint8_t *d_valid = dst_valid, *d_heap = (uint8_t *)dst_heap;
	DevBuf<uint4> tmp_cells;
	DevBuf<uint8_t> tmp_valid, tmp_heap;
	if (!to_device) {
		HIPCHK(ctx, tmp_cells.alloc(n));
		d_cells = tmp_cells;
		if (dst_valid) {
			HIPCHK(ctx, tmp_valid.alloc(n));
			d_valid = tmp_valid;
		}
		if (total) {
			HIPCHK(ctx, tmp_heap.alloc(total));
			d_heap = tmp_heap;
		}
	}
	polr_launch_strout_write(st, o, c.slot, c.dev, row_off.get(), chunk_heap_base, d_cells, d_valid, d_heap, (uint64_t)dst_heap);
	if (!to_device) {
		HIPCHK(ctx, hipMemcpyAsync(dst_cells, tmp_cells, n * 16, hipMemcpyDeviceToHost, st));
		if (dst_valid) {
			HIPCHK(ctx, hipMemcpyAsync(dst_valid, tmp_valid, n, hipMemcpyDeviceToHost, st));
		}
		if (total) {
			HIPCHK(ctx, hipMemcpyAsync(dst_heap, tmp_heap, total, hipMemcpyDeviceToHost, st));
		}
	}
	HIPCHK(ctx, hipStreamSynchronize(st)); // (the scratch and the staged copies are locals)
	return POLR_OK;
}
