// duckdb-polr_amd/csrc/polr_strheap.hip -- VARCHAR columns on the device: the upload of their string heaps
// (polr_ht_set_payload_heap(s), polr_pipeline_set_probe_heap(s)), the guard of a column whose heap never came
// (check_string_col_on_device, polr_internal.h), the MIN / MAX sink over string_t cells (polr_out_aggregate_string) and the
// one path by which strings leave the device as records (polr_fetch_str_records, polr_internal.h; polr_strrec_plan.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "polr_internal.h"
#include "polr_strcmp.h"
#include "polr_strrec_plan.h"

// ---- VARCHAR: string heaps on the device and the MIN / MAX sink over string_t cells -------------------------------------
// (string_type.hpp:23-28: {u32 length, char inlined[12]} or {u32 length, char prefix[4], char *ptr})
// one host range of a heap and where its copy lives on the device; a column's ranges sorted by host_base, disjoint
struct HeapRange {
	uint64_t host_base, bytes, dev_base;
};

// the range that holds all of [ptr, ptr + len), or -1 (ranges sorted and disjoint: at most one can)
__device__ __forceinline__ int find_heap_range(const HeapRange *r, uint32_t n, uint64_t ptr, uint32_t len) {
	uint32_t lo = 0, hi = n; // -> the first range whose host_base lies above ptr
	while (lo < hi) {
		const uint32_t mid = (lo + hi) / 2;
		if (r[mid].host_base <= ptr) {
			lo = mid + 1;
		} else {
			hi = mid;
		}
	}
	if (lo == 0) {
		return -1;
	}
	const HeapRange &h = r[lo - 1];
	return (len <= h.bytes && ptr - h.host_base <= h.bytes - len) ? (int)(lo - 1) : -1; // (no wrap-around at 2^64)
}

// rewrite = 0: count the non-NULL long cells that no range holds; rewrite = 1 (after a count of 0): rebase those cells onto
// the device copies and zero the cells of NULL rows (the reference leaves them uninitialised: nothing may follow them)
__global__ __launch_bounds__(256) void polr_rebase_strings_kernel(uint4 *cells, const uint8_t *__restrict__ valid, uint64_t n,
                                                                  const HeapRange *__restrict__ ranges, uint32_t n_ranges,
                                                                  int rewrite, unsigned long long *outside) {
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) {
		return;
	}
	if (valid && !valid[i]) {
		if (rewrite) {
			cells[i] = make_uint4(0, 0, 0, 0);
		}
		return;
	}
	uint4 c = cells[i];
	if (c.x <= 12u) {
		return;
	}
	const uint64_t ptr = ((uint64_t)c.w << 32) | c.z;
	const int r = find_heap_range(ranges, n_ranges, ptr, c.x);
	if (r < 0) {
		if (!rewrite) {
			atomicAdd(outside, 1ull); // (a cell pointing outside the heap it was said to live in)
		}
		return;
	}
	if (rewrite) {
		const uint64_t moved = ptr - ranges[r].host_base + ranges[r].dev_base;
		c.z = (uint32_t)moved;
		c.w = (uint32_t)(moved >> 32);
		cells[i] = c;
	}
}

// a < b in the order of the reference's string comparison: unsigned bytes, a proper prefix first
__device__ __forceinline__ bool str_less(const uint4 &a, const uint4 &b) {
	const uint32_t n = a.x < b.x ? a.x : b.x;
	// the first four characters sit in the same place in both forms
	const uint32_t pa = __builtin_bswap32(a.y), pb = __builtin_bswap32(b.y);
	if (n >= 4 && pa != pb) {
		return pa < pb;
	}
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t x = str_byte(a, i), y = str_byte(b, i);
		if (x != y) {
			return x < y;
		}
	}
	return a.x < b.x;
}

struct StrPartial {
	uint4 cell;
	uint32_t have;
	uint32_t pad[3];
};

// phase 1: per workgroup the extreme of its share of the output rows; phase 2 (one workgroup, n_in partials): the extreme
__global__ __launch_bounds__(256) void polr_agg_string_kernel(DevOut out, uint32_t n_chunks, DevCol src, uint32_t slot, int want_max,
                                                              const StrPartial *__restrict__ in, uint32_t n_in,
                                                              StrPartial *__restrict__ partials) {
	__shared__ StrPartial wave_part[4];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	uint4 best = make_uint4(0, 0, 0, 0);
	bool have = false;
	auto offer = [&](const uint4 &c) {
		if (!have || (want_max ? str_less(best, c) : str_less(c, best))) {
			best = c;
			have = true;
		}
	};
	if (in) {
		for (uint32_t i = threadIdx.x; i < n_in; i += blockDim.x) {
			if (in[i].have) {
				offer(in[i].cell);
			}
		}
	} else {
		for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
			const uint32_t n = out.chunk_count[chunk];
			const uint32_t *ids = out.ids + (uint64_t)slot * out.slot_stride + (uint64_t)chunk * out.chunk_capacity;
			for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
				const uint32_t row = ids[i];
				if (src.valid && !src.valid[row]) {
					continue; // NULLs take no part
				}
				offer(((const uint4 *)src.data)[row]);
			}
		}
	}
	for (int d = 32; d > 0; d >>= 1) {
		uint4 o;
		o.x = __shfl_down(best.x, d, 64);
		o.y = __shfl_down(best.y, d, 64);
		o.z = __shfl_down(best.z, d, 64);
		o.w = __shfl_down(best.w, d, 64);
		const bool ohave = __shfl_down(have ? 1 : 0, d, 64) != 0;
		if (ohave && (int)lane + d < 64) {
			offer(o);
		}
	}
	if (lane == 0) {
		wave_part[wave].cell = best;
		wave_part[wave].have = have ? 1u : 0u;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		have = false;
		for (uint32_t w = 0; w < (blockDim.x >> 6); w++) {
			if (wave_part[w].have) {
				offer(wave_part[w].cell);
			}
		}
		StrPartial r;
		r.cell = best;
		r.have = have ? 1u : 0u;
		r.pad[0] = r.pad[1] = r.pad[2] = 0;
		partials[blockIdx.x] = r;
	}
}

// the guard of a VARCHAR column whose cells were never rebased onto a device heap: the non-NULL cells among the output rows
// that are longer than 12 bytes -- their pointers are the host's.  Reads the length word of a cell and nothing else.
__global__ __launch_bounds__(256) void polr_count_long_cells_kernel(DevOut out, uint32_t n_chunks, DevCol src, uint32_t slot,
                                                                    unsigned long long *__restrict__ n_long) {
	unsigned long long mine = 0;
	for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
		const uint32_t n = out.chunk_count[chunk];
		const uint32_t *ids = out.ids + (uint64_t)slot * out.slot_stride + (uint64_t)chunk * out.chunk_capacity;
		for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
			const uint32_t row = ids[i];
			if (src.valid && !src.valid[row]) {
				continue;
			}
			mine += *(const uint32_t *)(src.data + (uint64_t)row * 16u) > 12u ? 1u : 0u;
		}
	}
	mine = wave_sum64(mine);
	if ((threadIdx.x & 63u) == 0 && mine) {
		atomicAdd(n_long, mine);
	}
}

// POLR_OK when the column may be read by a kernel that follows string pointers
int check_string_col_on_device(polr_out *o, hipStream_t st, const OutCol &c, const char *what, uint32_t idx) {
	polr_ctx *ctx = o->pipe->ctx;
	if (c.col->strings_rebased || !c.col->owned() || o->n_chunks == 0) {
		return POLR_OK; // (rebased here; or the caller's own device memory, whose cells point into HBM by contract)
	}
	DevBuf<unsigned long long> n_long;
	unsigned long long h_long = 0;
	HIPCHK(ctx, n_long.alloc(1));
	HIPCHK(ctx, hipMemsetAsync(n_long, 0, 8, st));
	const uint32_t n_blocks = std::max<uint32_t>(1, std::min<uint32_t>(o->n_chunks, (uint32_t)ctx->n_cus * 4));
	hipLaunchKernelGGL(polr_count_long_cells_kernel, dim3(n_blocks), dim3(256), 0, st, o->dev, o->n_chunks, c.dev, c.slot, n_long.get());
	HIPCHK(ctx, hipMemcpyAsync(&h_long, n_long, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	if (h_long) {
		POLR_FAIL_HEAP_NEVER_CAME(ctx, what, idx, h_long);
	}
	return POLR_OK;
}

// ---- string records: how strings leave the device (polr_strrec_plan.h) -------------------------------------------------
// the bytes of the string of cell c through str_byte.  INLINE says which form the cell has (length <= 12, or prefix and
// pointer), so that the loop is compiled once per form -- str_byte folds to the word shift or to the pointer read --
// instead of deciding it for every byte
template <bool INLINE>
__device__ __forceinline__ void str_record_bytes(uint8_t *__restrict__ dst, const uint4 &c) {
	__builtin_assume(INLINE ? c.x <= 12u : c.x > 12u);
	for (uint32_t j = 0; j < c.x; j++) {
		dst[j] = (uint8_t)str_byte(c, j);
	}
}

// record i {u32 length, bytes} of the string of cell cells[index ? index[i] : i], at the offset the host laid out
__global__ __launch_bounds__(256) void polr_str_records_kernel(const uint4 *__restrict__ cells, const uint32_t *__restrict__ index,
                                                               const uint64_t *__restrict__ offsets, uint64_t n,
                                                               uint8_t *__restrict__ arena, uint64_t arena_bytes) {
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) {
		return;
	}
	const uint64_t off = offsets[i];
	if (off == POLR_STRREC_NONE) {
		return; // (no record: the cell may hold anything and is not read)
	}
	const uint4 c = cells[index ? index[i] : i];
	if (off > arena_bytes || arena_bytes - off < 4ull + c.x) {
		return; // (never past the arena, whatever the offsets say)
	}
	uint8_t *dst = arena + off;
	for (uint32_t j = 0; j < 4; j++) {
		dst[j] = (uint8_t)(c.x >> (8u * j));
	}
	if (c.x <= 12u) {
		str_record_bytes<true>(dst + 4, c);
	} else {
		str_record_bytes<false>(dst + 4, c);
	}
}

int polr_fetch_str_records(polr_ctx *ctx, hipStream_t st, const uint4 *d_cells, const uint32_t *d_index, uint64_t n,
                           const uint64_t *offs, uint64_t used, uint64_t n_offsets, uint64_t *d_offs, uint8_t *str_bytes,
                           uint64_t str_cap) {
	if (!polr_strrec_fits(used, str_cap, n, n_offsets)) {
		return POLR_E_OVERFLOW;
	}
	if (used == 0) {
		return POLR_OK; // (no entry has a record)
	}
	DevBuf<uint8_t> arena;
	DevBuf<uint64_t> own_offs;
	HIPCHK(ctx, arena.alloc(used));
	if (!d_offs) {
		HIPCHK(ctx, own_offs.alloc(n));
		d_offs = own_offs;
	}
	HIPCHK(ctx, hipMemcpyAsync(d_offs, offs, n * 8, hipMemcpyHostToDevice, st));
	hipLaunchKernelGGL(polr_str_records_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_cells, d_index,
	                   (const uint64_t *)d_offs, n, arena.get(), used);
	HIPCHK(ctx, hipMemcpyAsync(str_bytes, arena, used, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	return POLR_OK;
}

// all or nothing: the ranges are checked, copied and every cell validated before any cell is rewritten; on an error the
// column is as it was and no device memory is kept
static int set_string_heaps(polr_ctx *ctx, OwnedCol *c, uint64_t n_rows, const polr_heap_range *ranges, uint32_t n_ranges,
                            std::vector<DevBuf<uint8_t>> &owner) {
	if (!ranges || n_ranges == 0) {
		POLR_FAIL(ctx, POLR_E_INVALID, "a string heap needs at least one range");
	}
	if (c->width != 16) {
		POLR_FAIL(ctx, POLR_E_INVALID, "a string heap belongs to a column of 16-byte string cells (this one: %u bytes)", c->width);
	}
	if (c->strings_rebased) {
		POLR_FAIL(ctx, POLR_E_INVALID, "the column's string cells point into a device heap already");
	}
	std::vector<HeapRange> hr(n_ranges);
	std::vector<uint32_t> order(n_ranges);
	uint64_t total = 0;
	for (uint32_t r = 0; r < n_ranges; r++) {
		const uint64_t base = (uint64_t)ranges[r].base, bytes = ranges[r].bytes;
		if (!base || bytes == 0 || base + bytes < base) {
			POLR_FAIL(ctx, POLR_E_INVALID, "heap range %u: empty, NULL or past the end of the address space", r);
		}
		order[r] = r;
		total += bytes;
	}
	std::sort(order.begin(), order.end(),
	          [&](uint32_t a, uint32_t b) { return (uint64_t)ranges[a].base < (uint64_t)ranges[b].base; });
	uint64_t at = 0;
	for (uint32_t r = 0; r < n_ranges; r++) {
		const polr_heap_range &x = ranges[order[r]];
		if (r && (uint64_t)x.base < hr[r - 1].host_base + hr[r - 1].bytes) {
			POLR_FAIL(ctx, POLR_E_INVALID, "heap ranges %u and %u overlap", order[r - 1], order[r]);
		}
		hr[r].host_base = (uint64_t)x.base;
		hr[r].bytes = x.bytes;
		hr[r].dev_base = at; // (offset for now: the device address once the copy exists)
		at += x.bytes;
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	DevBuf<uint8_t> heap;
	DevBuf<HeapRange> d_ranges;
	DevBuf<unsigned long long> outside;
	HIPCHK(ctx, heap.alloc(total));
	HIPCHK(ctx, d_ranges.alloc(n_ranges));
	HIPCHK(ctx, outside.alloc(1));
	for (uint32_t r = 0; r < n_ranges; r++) {
		HIPCHK(ctx, hipMemcpyAsync(heap + hr[r].dev_base, (const void *)hr[r].host_base, hr[r].bytes, hipMemcpyHostToDevice, ctx->stream));
		hr[r].dev_base += (uint64_t)heap.get();
	}
	HIPCHK(ctx, hipMemcpyAsync(d_ranges, hr.data(), n_ranges * sizeof(HeapRange), hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipMemsetAsync(outside, 0, 8, ctx->stream));
	const dim3 grid((unsigned)((n_rows + 255) / 256));
	if (n_rows) {
		hipLaunchKernelGGL(polr_rebase_strings_kernel, grid, dim3(256), 0, ctx->stream, (uint4 *)c->data, c->valid, n_rows,
		                   d_ranges.get(), n_ranges, 0, outside.get());
	}
	unsigned long long bad = 0;
	HIPCHK(ctx, hipMemcpyAsync(&bad, outside, 8, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	if (bad) {
		POLR_FAIL(ctx, POLR_E_INVALID, "%llu non-NULL string cells point outside the heap ranges given for their column", bad);
	}
	if (n_rows) {
		hipLaunchKernelGGL(polr_rebase_strings_kernel, grid, dim3(256), 0, ctx->stream, (uint4 *)c->data, c->valid, n_rows,
		                   d_ranges.get(), n_ranges, 1, outside.get());
		HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	}
	owner.push_back(std::move(heap)); // (only now: a refused call keeps nothing)
	c->strings_rebased = true;
	return POLR_OK;
}

extern "C" {

int polr_ht_set_payload_heaps(polr_ht *ht, uint32_t payload_col, const polr_heap_range *ranges, uint32_t n_ranges) {
	POLR_ENTRY();
	if (!ht || payload_col >= ht->n_payload) {
		return POLR_E_INVALID;
	}
	if (ht->kind != KIND_NONE) {
		// (a finalized perfect table keeps a re-ordered copy of every payload column: rebase before finalizing)
		POLR_FAIL(ht->ctx, POLR_E_INVALID, "set the string heap of a payload column before the table is finalized");
	}
	return set_string_heaps(ht->ctx, &ht->payload[payload_col], ht->n_rows_in, ranges, n_ranges, ht->heaps);
}

int polr_ht_set_payload_heap(polr_ht *ht, uint32_t payload_col, const void *heap_base, uint64_t heap_bytes) {
	const polr_heap_range r = {heap_base, heap_bytes};
	return polr_ht_set_payload_heaps(ht, payload_col, &r, 1);
}

int polr_pipeline_set_probe_heaps(polr_pipeline *p, uint32_t probe_col, const polr_heap_range *ranges, uint32_t n_ranges) {
	POLR_ENTRY();
	if (!p || probe_col >= p->n_probe_cols) {
		return POLR_E_INVALID;
	}
	if (!p->probe_cols[probe_col].owned()) {
		POLR_FAIL(p->ctx, POLR_E_INVALID, "probe column %u lives in the caller's device memory: its cells must point into HBM already",
		          probe_col);
	}
	return set_string_heaps(p->ctx, &p->probe_cols[probe_col], p->n_probe_rows, ranges, n_ranges, p->heaps);
}

int polr_pipeline_set_probe_heap(polr_pipeline *p, uint32_t probe_col, const void *heap_base, uint64_t heap_bytes) {
	const polr_heap_range r = {heap_base, heap_bytes};
	return polr_pipeline_set_probe_heaps(p, probe_col, &r, 1);
}

int polr_out_aggregate_string(polr_out *o, void *stream, uint32_t fn, int32_t src_join, uint32_t src_col, char *dst,
                              uint32_t dst_cap, uint32_t *len, uint32_t *is_null) {
	POLR_ENTRY();
	if (!o || !len || !is_null || (!dst && dst_cap)) {
		return POLR_E_INVALID;
	}
	polr_pipeline *p = o->pipe;
	polr_ctx *ctx = p->ctx;
	POLR_REFUSE_AGG_CELLS(ctx, o);
	if (fn != POLR_AGG_MIN && fn != POLR_AGG_MAX) {
		POLR_FAIL(ctx, POLR_E_UNSUPPORTED, "string aggregate %u (MIN or MAX)", fn);
	}
	OutCol c;
	int rc = polr_out_col(p, src_join, src_col, &c, "string aggregate, column", src_col);
	if (rc) {
		return rc;
	}
	if (c.dev.width != 16) {
		POLR_FAIL(ctx, POLR_E_INVALID, "not a VARCHAR column (%u-byte cells)", c.dev.width);
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	rc = out_ensure_stats(o, stream);
	if (rc) {
		return rc;
	}
	*len = 0;
	*is_null = 1;
	if (o->n_chunks == 0) {
		return POLR_OK;
	}
	// a column whose heap never came may hold inline strings only: refused before a pointer is followed
	rc = check_string_col_on_device(o, st, c, "string aggregate, column", src_col);
	if (rc) {
		return rc;
	}
	const uint32_t n_blocks = std::max<uint32_t>(1, std::min<uint32_t>(o->n_chunks, (uint32_t)ctx->n_cus * 4));
	DevBuf<StrPartial> part_mem;
	HIPCHK(ctx, part_mem.alloc((size_t)n_blocks + 1));
	StrPartial *part = part_mem;
	hipLaunchKernelGGL(polr_agg_string_kernel, dim3(n_blocks), dim3(256), 0, st, o->dev, o->n_chunks, c.dev, c.slot,
	                   fn == POLR_AGG_MAX ? 1 : 0, (const StrPartial *)nullptr, 0u, part);
	hipLaunchKernelGGL(polr_agg_string_kernel, dim3(1), dim3(256), 0, st, o->dev, 0u, c.dev, c.slot, fn == POLR_AGG_MAX ? 1 : 0,
	                   (const StrPartial *)part, n_blocks, part + n_blocks);
	StrPartial win;
	hipError_t e = hipMemcpyAsync(&win, part + n_blocks, sizeof(win), hipMemcpyDeviceToHost, st);
	e = e == hipSuccess ? hipStreamSynchronize(st) : e;
	if (e == hipSuccess && win.have) {
		*is_null = 0;
		*len = win.cell.x;
		const uint32_t take = std::min<uint32_t>(win.cell.x, dst_cap);
		if (win.cell.x <= 12) {
			const uint32_t words[3] = {win.cell.y, win.cell.z, win.cell.w};
			memcpy(dst, words, take);
		} else if (take) {
			e = hipMemcpy(dst, (const void *)(((uint64_t)win.cell.w << 32) | win.cell.z), take, hipMemcpyDeviceToHost);
		}
	}
	if (e != hipSuccess) {
		POLR_FAIL(ctx, POLR_E_HIP, "string aggregate failed: %s", hipGetErrorString(e));
	}
	return POLR_OK;
}

} // extern "C"
