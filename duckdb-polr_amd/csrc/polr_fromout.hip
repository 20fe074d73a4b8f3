// duckdb-polr_amd/csrc/polr_fromout.hip -- polr_ht_from_output: the output of one pipeline as the un-finalized build side
// of another hash join, built on the device (a pipeline whose sink is PhysicalHashJoin::Sink, physical_hash_join.cpp:217-286).
// Build row r of the new table is output row r, chunk-major as polr_out_fetch_ids numbers them.  Contract:
// include/polr_hip.h; the request checked and laid out: polr_fromout_plan.h.
//
// Fixed-width columns (1, 2, 4, 8 bytes), keys and payload alike, are gathered by ONE launch: a workgroup per output chunk
// and slot group, a lane per output row -- four rows a lane at a time, a block width apart, so that four independent
// gathers are in flight per lane and a column's descriptor is read once for all of them.  The columns come ordered by the
// slot of row ids that indexes their source and a workgroup serves the columns of ONE slot: a lane loads that slot's row
// id once and serves every column of the slot with it.  Per column it loads the validity byte if the source has one, the
// cell only when the row is valid, and stores cell and validity at the row's own index: consecutive lanes write
// consecutive cells (coalesced stores; the loads are gathers by nature).  The slot group is the slow index of the grid,
// so the workgroups on the device at one time gather from one source table, not from all of them: with every slot in one
// workgroup the build columns of all joins competed for the L2 at once and the launch was slower than one launch per
// column (1.16 ms against 0.83 ms on the workload of tools/bench_from_output.py; slot by slot 0.90 ms).  The column
// descriptors -- up to 66 -- lie in a device array read through the constant address space: scalar loads, the same for
// the whole wave, no vector register holds them.
// Algorithmic bytes per output row: 4 read per distinct slot; w + 1 read and w + 1 written per column of w bytes.
// gfx950: 30 VGPRs, 70 SGPRs, no scratch, no LDS, no spills (the kernel's metadata note, llvm-readelf --notes of the code
// object); the descriptors arrive through s_load, every other access is global_load / global_store.
//
// VARCHAR payload columns go through the measure and write passes of polr_strout.hip: every column is measured first, the
// totals and long-cell counts of all of them are read back once, the heap-never-came guard is decided, then the heaps --
// one DevBuf per column, owned by the table -- are allocated with everything else the table holds, and only then does the
// first kernel write into the table.  The cells and validity arrays of ALL columns and the gather's descriptors share one
// allocation (polr_ht::col_mem; the plan places them), and the string passes share one scratch allocation: nothing but
// that scratch is freed inside the call.
//
// The device part -- measuring the VARCHAR columns, the gather launch, the string write passes -- is shared with
// polr_pipeline_from_output (polr_pipesrc.hip), whose columns become the probe side of a new pipeline instead of a table:
// polr_fromout_measure / polr_fromout_fill below, declared in polr_fromout_gather.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <memory>
#include <vector>

#include "polr_fromout_gather.h"


typedef PolrFromoutDesc FromoutCol;

#define FROMOUT_R 4 // output rows a lane serves per column: that many independent gathers in flight

// R rows of one column: all validity bytes first, then the cells of the valid rows, then the stores
template <class T>
__device__ __forceinline__ void fromout_cells(const POLR_GLOBAL uint8_t *src_valid, const POLR_GLOBAL uint8_t *src,
                                              POLR_GLOBAL uint8_t *dst, POLR_GLOBAL uint8_t *dst_valid, const uint32_t (&row)[FROMOUT_R],
                                              const bool (&live)[FROMOUT_R], uint64_t at, uint32_t step) {
	bool valid[FROMOUT_R];
	T v[FROMOUT_R];
#pragma unroll
	for (int r = 0; r < FROMOUT_R; r++) {
		valid[r] = live[r] && (!src_valid || src_valid[row[r]] != 0);
	}
#pragma unroll
	for (int r = 0; r < FROMOUT_R; r++) {
		v[r] = 0;
		if (valid[r]) {
			v[r] = ((const POLR_GLOBAL T *)src)[row[r]];
		}
	}
#pragma unroll
	for (int r = 0; r < FROMOUT_R; r++) {
		if (live[r]) {
			((POLR_GLOBAL T *)dst)[at + (uint64_t)r * step] = v[r];
			dst_valid[at + (uint64_t)r * step] = valid[r] ? 1 : 0;
		}
	}
}

struct FromoutGroups { // cols[first[g] .. first[g + 1]) are the columns of slot group g
	uint32_t first[POLR_FROMOUT_MAX_SLOTS + 1];
};

// cols[] ordered by slot; dst row = chunk_base[chunk] + position in the chunk.  Grid: x the chunk, y the slot group, so
// that the workgroups on the device at one time gather from the columns of ONE source table (x runs fastest).  A chunk is
// served in tiles of FROMOUT_R * blockDim.x rows: lane t has the rows tile + t, tile + blockDim.x + t, ... (consecutive
// lanes, consecutive rows); the row ids of a tile are loaded once, a column's descriptor once per tile.
__global__ __launch_bounds__(256) void polr_fromout_gather_kernel(DevOut out, const uint64_t *__restrict__ chunk_base_,
                                                                   uint32_t n_chunks, const FromoutCol *__restrict__ cols_,
                                                                   FromoutGroups groups) {
	const uint32_t chunk = blockIdx.x;
	if (chunk >= n_chunks) {
		return;
	}
	const uint32_t c_begin = groups.first[blockIdx.y], c_end = groups.first[blockIdx.y + 1];
	const uint32_t n = as_global(out.chunk_count)[chunk];
	const uint64_t base = as_global(chunk_base_)[chunk];
	const POLR_CONST FromoutCol *cols = (const POLR_CONST FromoutCol *)cols_;
	const POLR_GLOBAL uint32_t *ids =
	    as_global(out.ids) + (uint64_t)cols[c_begin].slot * out.slot_stride + (uint64_t)chunk * out.chunk_capacity;
	const uint32_t step = blockDim.x;
	for (uint32_t tile = 0; tile < n; tile += FROMOUT_R * step) {
		const uint32_t first = tile + threadIdx.x;
		bool live[FROMOUT_R];
		uint32_t row[FROMOUT_R];
#pragma unroll
		for (int r = 0; r < FROMOUT_R; r++) {
			live[r] = first + r * step < n;
			row[r] = 0;
			if (live[r]) {
				row[r] = ids[first + r * step];
			}
		}
		const uint64_t at = base + first;
		for (uint32_t c = c_begin; c < c_end; c++) {
			const POLR_CONST FromoutCol *d = cols + c;
			const POLR_GLOBAL uint8_t *sv = as_global(d->src_valid);
			const POLR_GLOBAL uint8_t *sd = as_global(d->src_data);
			POLR_GLOBAL uint8_t *dd = as_global(d->dst_data);
			POLR_GLOBAL uint8_t *dv = as_global(d->dst_valid);
			switch (d->width) {
			case 1:
				fromout_cells<uint8_t>(sv, sd, dd, dv, row, live, at, step);
				break;
			case 2:
				fromout_cells<uint16_t>(sv, sd, dd, dv, row, live, at, step);
				break;
			case 4:
				fromout_cells<uint32_t>(sv, sd, dd, dv, row, live, at, step);
				break;
			default:
				fromout_cells<uint64_t>(sv, sd, dd, dv, row, live, at, step);
				break;
			}
		}
	}
}

PolrFromoutColumn polr_fromout_shape(const OutCol &c) {
	PolrFromoutColumn s;
	s.resolved = 1;
	s.slot = c.slot;
	s.width = c.dev.width;
	s.flags = c.dev.flags & POLR_COL_SIGNED;
	s.has_valid = c.dev.valid != nullptr;
	s.owned = c.col->owned();
	s.rebased = c.col->strings_rebased;
	return s;
}

int polr_fromout_measure(polr_out *o, hipStream_t st, const PolrFromoutPlan &plan, const OutCol *src, uint64_t n, uint32_t nc,
                         FromoutStrings &fs) {
	polr_ctx *ctx = o->ctx;
	const size_t ns = plan.strings.size();
	const uint64_t cw = 2ull * nc; // chunk_words, per column: [nc] byte totals, [nc] their exclusive prefix
	fs.h_tails.assign(2 * ns, 0);
	if (!ns || !n) {
		return POLR_OK;
	}
	HIPCHK(ctx, fs.scratch.alloc(plan.row_off_words + plan.chunk_words + plan.tail_words));
	fs.row_off = fs.scratch.get();
	fs.chunk_words = fs.row_off + plan.row_off_words;
	fs.tails = fs.chunk_words + plan.chunk_words;
	HIPCHK(ctx, hipMemsetAsync(fs.tails, 0, plan.tail_words * 8, st));
	for (size_t s = 0; s < ns; s++) {
		uint64_t *chunk_bytes = fs.chunk_words + s * cw, *chunk_heap_base = chunk_bytes + nc, *tail = fs.tails + 2 * s;
		polr_launch_strout_measure(st, o, plan.strings[s].slot, src[plan.strings[s].col].dev, fs.row_off + s * n, chunk_bytes,
		                           (unsigned long long *)(tail + 1));
		polr_launch_chunk_prefix(st, (const uint64_t *)chunk_bytes, nc, chunk_heap_base, tail);
	}
	HIPCHK(ctx, hipMemcpyAsync(fs.h_tails.data(), fs.tails, plan.tail_words * 8, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	return POLR_OK;
}

int polr_fromout_fill(polr_out *o, hipStream_t st, const PolrFromoutPlan &plan, const OutCol *src, uint64_t n, uint32_t nc,
                      const FromoutStrings &fs, uint8_t *mem, const std::vector<DevBuf<uint8_t>> &heaps,
                      std::vector<PolrFromoutDesc> &h_desc) {
	polr_ctx *ctx = o->ctx;
	if (!n) {
		return POLR_OK;
	}
	h_desc.resize(plan.fixed.size());
	FromoutCol *desc = (FromoutCol *)(mem + plan.desc_off);
	for (size_t i = 0; i < plan.fixed.size(); i++) {
		const uint32_t c = plan.fixed[i].col;
		h_desc[i] = FromoutCol{src[c].dev.data, src[c].dev.valid, mem + plan.data_off[c], mem + plan.valid_off[c], plan.fixed[i].width,
		                       plan.fixed[i].slot};
	}
	if (!h_desc.empty()) {
		HIPCHK(ctx, hipMemcpyAsync(desc, h_desc.data(), h_desc.size() * sizeof(FromoutCol), hipMemcpyHostToDevice, st));
		FromoutGroups groups = {};
		for (uint32_t g = 0; g <= plan.n_slots; g++) {
			groups.first[g] = plan.group_first[g];
		}
		hipLaunchKernelGGL(polr_fromout_gather_kernel, dim3(nc, plan.n_slots), dim3(polr_strout_block(o)), 0, st, o->dev,
		                   o->chunk_base.get(), nc, desc, groups);
	}
	const uint64_t cw = 2ull * nc;
	for (size_t s = 0; s < plan.strings.size(); s++) {
		const uint32_t c = plan.strings[s].col;
		const uint64_t *chunk_heap_base = fs.chunk_words + s * cw + nc;
		uint8_t *heap = heaps[s].get();
		polr_launch_strout_write(st, o, plan.strings[s].slot, src[c].dev, fs.row_off + s * n, chunk_heap_base,
		                         (uint4 *)(mem + plan.data_off[c]), mem + plan.valid_off[c], heap, (uint64_t)heap);
	}
	return POLR_OK;
}

extern "C" int polr_ht_from_output(polr_out *o, void *stream, const polr_out_col_ref *keys, uint32_t n_keys,
                                   const polr_out_col_ref *payload, uint32_t n_payload, polr_ht **out) {
	POLR_ENTRY();
	if (out) {
		*out = nullptr;
	}
	if (!o) {
		return POLR_E_INVALID;
	}
	polr_pipeline *p = o->pipe;
	polr_ctx *ctx = p->ctx;
	// refusals before anything is enqueued (the output's own statistics apart)
	PolrFromoutRequest rq = {};
	rq.has_out = true;
	rq.has_result = out != nullptr;
	rq.has_keys = keys != nullptr;
	rq.has_payload = payload != nullptr;
	rq.fused = out_has_fused_sink(o);
	rq.n_keys = n_keys;
	rq.n_payload = n_payload;
	PolrFromoutPlan plan;
	int rc = polr_fromout_check(rq, plan);
	if (rc) {
		POLR_FAIL(ctx, rc, "%s", plan.err);
	}
	const uint32_t n_cols = n_keys + n_payload;
	std::vector<OutCol> src(n_cols);
	std::vector<PolrFromoutColumn> shapes(n_cols);
	for (uint32_t c = 0; c < n_cols; c++) {
		const bool is_key = c < n_keys;
		const polr_out_col_ref &r = is_key ? keys[c] : payload[c - n_keys];
		POLR_TRY(polr_out_col(p, r.src_join, r.src_col, &src[c], is_key ? "key" : "payload column", is_key ? c : c - n_keys));
		shapes[c] = polr_fromout_shape(src[c]);
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	POLR_TRY(out_ensure_stats(o, stream));
	const uint64_t n = o->n_rows; // (0 also for an output no materialising run has filled)
	const uint32_t nc = n ? o->n_chunks : 0;
	rq.n_rows = n;
	rq.n_chunks = nc;
	rc = polr_fromout_plan(rq, shapes.data(), plan);
	if (rc) {
		POLR_FAIL(ctx, rc, "%s", plan.err);
	}
	// VARCHAR columns: measure all of them, read back once, decide the guard
	const size_t ns = plan.strings.size();
	FromoutStrings fs;
	POLR_TRY(polr_fromout_measure(o, st, plan, src.data(), n, nc, fs));
	for (size_t s = 0; s < ns; s++) {
		const uint64_t n_long = fs.h_tails[2 * s + 1];
		if (n_long && plan.strings[s].needs_heap_guard) {
			// (the library's own upload, never rebased onto a device heap: the pointers of its long cells are the host's)
			POLR_FAIL_HEAP_NEVER_CAME(ctx, "payload column", plan.strings[s].col - n_keys, n_long);
		}
	}
	// the table and everything it owns, before the first kernel that writes into it
	HandleGuard<polr_ht> ht = polr_ht_new(ctx, n_keys, n_payload, n);
	HIPCHK(ctx, ht->col_mem.alloc(plan.table_bytes));
	ht->device_bytes += ht->col_mem.bytes();
	for (uint32_t c = 0; c < n_cols; c++) {
		OwnedCol &col = c < n_keys ? ht->keys[c] : ht->payload[c - n_keys];
		col.width = shapes[c].width;
		col.flags = shapes[c].flags;
		col.data = ht->col_mem.get() + plan.data_off[c];
		col.valid = ht->col_mem.get() + plan.valid_off[c];
	}
	ht->heaps.reserve(ns);
	for (size_t s = 0; s < ns; s++) {
		DevBuf<uint8_t> heap;
		HIPCHK(ctx, heap.alloc(fs.h_tails[2 * s]));
		ht->device_bytes += heap.bytes();
		ht->heaps.push_back(std::move(heap));
		ht->payload[plan.strings[s].col - n_keys].strings_rebased = true;
	}
	ht->key_signed = ht->keys[0].flags & POLR_COL_SIGNED;
	std::vector<DevCol> h_keys(n_keys);
	for (uint32_t c = 0; c < n_keys; c++) {
		h_keys[c] = dev_col(ht->keys[c]);
	}
	HIPCHK(ctx, ht->keys_dev.alloc(n_keys));
	ht->device_bytes += ht->keys_dev.bytes();
	// fill it
	std::vector<FromoutCol> h_desc;
	HIPCHK(ctx, hipMemcpyAsync(ht->keys_dev.get(), h_keys.data(), n_keys * sizeof(DevCol), hipMemcpyHostToDevice, st));
	POLR_TRY(polr_fromout_fill(o, st, plan, src.data(), n, nc, fs, ht->col_mem.get(), ht->heaps, h_desc));
	HIPCHK(ctx, hipStreamSynchronize(st)); // (the table is complete; the staged descriptors and the scratch are locals)
	*out = ht.release();
	return POLR_OK;
}
