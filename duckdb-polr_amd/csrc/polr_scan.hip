// duckdb-polr_amd/csrc/polr_scan.hip -- the source side of the POLAR pipeline on the device.
//
// Reference: PhysicalTableScan hands the pipeline one DataChunk per STANDARD_VECTOR_SIZE-row vector of the
// table; pushed-down table filters (ConstantFilter / IS [NOT] NULL, AND-ed per column:
// src/storage/table/row_group.cpp:316-452 RowGroup::TemplatedScan, src/storage/table/column_segment.cpp:194-300
// TemplatedFilterSelection / FilterSelectionSwitch, :304-475 ColumnSegment::FilterSelection) thin every vector
// to the rows that pass, in row order; a vector with no survivor is skipped (row_group.cpp:399-416), a NULL
// never passes a comparison (column_segment.cpp:200).  The multiplexer therefore sees chunks of 1..V tuples.
//
// Here: three HBM-streaming passes; only the first reads the filter columns (already resident in HBM)
//   1. count   : one wave per vector, 64 rows per step: the row predicate and the LIP tests are evaluated, the survivors
//                counted with a ballot, and every step's ballot kept in the pipeline's pass-bit buffer (tscan_count).
//                One kernel per row predicate, so that an integer scan carries neither string nor program code:
//                  polr_tscan_count_kernel       DevFilterSet               polr_pipeline_scan_filter[_lip]
//                  polr_tscan_count_str_kernel   DevFilterSet + DevStrSet   polr_pipeline_scan_filter_str
//                  polr_tscan_count_expr_kernel  DevFxProg                  polr_pipeline_scan_filter_expr
//   2. scan    : exclusive prefix over the vectors of (tuples, non-empty vectors) packed in one u64
//                (per-1024-vector block sums -> one block scans the sums -> apply)
//   3. write   : polr_tscan_write_bits_kernel, one wave per vector again: ascending row ids to sel[] from the pass
//                bits, chunk boundary of every non-empty vector; evaluates nothing
// and the result -- selection + chunk boundaries -- stays on the device, installed in the pipeline; a
// multiplexer takes the boundaries with polr_mpx_use_scan_chunks.  Algorithmic bytes: the sum of the filter column
// widths [+ validity bytes, + LIP key widths] per table row, once, + 2 bits per row (the pass bit, written and read)
// + 4 per surviving row.
//
// VARCHAR constant comparisons (polr_pipeline_scan_filter_str; the reference pushes =, <, >, <=, >= against a VARCHAR
// constant and the prefix range of LIKE 'abc%' into the scan: filter_combiner.cpp:391-398, :426-485, evaluated on
// string_t by ColumnSegment::FilterSelection column_segment.cpp:435-442): a DevStrSet beside the integer filters.  A row
// costs one 16-byte cell load per distinct VARCHAR filter column; the comparison is polr_strcmp.h.  The heap is read only
// for a cell longer than 12 bytes whose first four bytes tie with a constant's.
//
// Filter expressions (polr_pipeline_scan_filter_expr; what the reference evaluates in a PhysicalFilter between the scan
// and the first join -- OR / NOT trees, IN lists, LIKE): a postfix program evaluated per row (see "expression filters"
// below; the program is checked and lowered by polr_filter_plan.h, LIKE is polr_like.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "polr_filter_plan.h"
#include "polr_fx_device.h" // int_cmp_holds, DevFxProg, fx_row_true
#include "polr_internal.h"
#include "polr_like.h"
#include "polr_strcmp.h"

struct DevFilter {
	const uint8_t *data;
	const uint8_t *valid;
	uint32_t width;
	uint32_t is_signed;
	uint32_t op;
	uint32_t pad;
	int64_t constant;
};

#define POLR_MAX_FILTERS 8
struct DevFilterSet {
	DevFilter f[POLR_MAX_FILTERS];
	uint32_t n;
	uint32_t pad;
};

// The VARCHAR comparisons of a scan, grouped by column on the host: column c is compared against cmp[first .. first + n),
// so the cell of a row is loaded once however many constants it meets (a LIKE range is two).  The constants travel by
// value -- length and first 12 bytes (polr_str_const) --; the bytes beyond 12 of the long ones lie in the pipeline's
// scan_str_tails buffer at tail_off.
struct DevStrCmp {
	polr_str_const c;
	uint32_t op; // POLR_CMP_EQ .. POLR_CMP_GE
	uint32_t tail_off;
};
struct DevStrCol {
	const uint8_t *data;
	const uint8_t *valid;
	uint32_t first, n;
};
struct DevStrSet {
	DevStrCol col[POLR_MAX_FILTERS];
	DevStrCmp cmp[POLR_MAX_FILTERS];
	const uint8_t *tails;
	uint32_t n_cols;
	uint32_t pad;
};

// LIP (lookahead information passing, the reference's `PRAGMA enable_lip`): the filters of the joins further up the
// pipeline are applied to the source chunks before they enter it (PipelineExecutor::FetchFromSource,
// src/parallel/pipeline_executor.cpp:396-465 -> PhysicalHashJoin::ProbeBloomFilter, physical_hash_join.cpp:579-635).
// The reference probes a bloom filter per eligible join (single condition, key traced back to a source column, filtered
// build side: physical_join.cpp:57-107) in an order it re-sorts by miss rate every 64 chunks; the order changes the
// work, never the survivors.  Here the "filter" of a join is its own index -- bit table, unique-key or run hash table:
// a bloom filter without false positives -- evaluated for the rows that pass the table filters, cheapest first.
struct DevLip {
	const uint8_t *key_data;
	const uint8_t *key_valid;
	const void *table;
	uint64_t mask;
	int64_t min_value;
	uint64_t range;
	uint32_t key_width, key_signed, kind;
	uint32_t sentinel_count; // S16: build rows whose key is the slots' empty marker (kept beside the table)
};
struct DevLipSet {
	DevLip f[POLR_KMAX];
	uint32_t n;
	uint32_t pad;
};

__device__ __forceinline__ bool lip_contains(const DevLip &f, uint64_t row) {
	if (f.key_valid && !f.key_valid[row]) {
		return false; // NULL never joins
	}
	const uint64_t key = load_cell(as_global(f.key_data) + row * f.key_width, f.key_width, f.key_signed && f.kind == KIND_PERFECT);
	if (f.kind == KIND_PERFECT) {
		uint64_t idx;
		return perfect_index(key, f.key_signed != 0, f.min_value, f.range, idx) &&
		       ((as_global((const uint32_t *)f.table)[idx >> 5] >> (idx & 31)) & 1u);
	}
	if (f.kind == KIND_S8) {
		const uint2 *tab = (const uint2 *)f.table; // {key32, row}
		const uint32_t k32 = (uint32_t)key;
		uint64_t h = polr_murmurhash64((uint64_t)k32) & f.mask;
		while (true) {
			const uint2 e = tab[h];
			if (e.y == S8_EMPTY_ROW) {
				return false;
			}
			if (e.x == k32) {
				return true;
			}
			h = (h + 1) & f.mask;
		}
	}
	// KIND_S16: {key64, start, count}
	if (key == S16_EMPTY_KEY) {
		return f.sentinel_count != 0; // (the all-ones key is the empty marker: its rows are counted beside the table)
	}
	const uint4 *tab = (const uint4 *)f.table;
	uint64_t h = polr_murmurhash64(key) & f.mask;
	while (true) {
		const uint4 e = tab[h];
		const uint64_t k = ((uint64_t)e.y << 32) | e.x;
		if (k == S16_EMPTY_KEY) {
			return false;
		}
		if (k == key) {
			return e.w != 0;
		}
		h = (h + 1) & f.mask;
	}
}

#define PACK_SHIFT 40 // low 40 bits: tuples, high 24: non-empty vectors
#define PACK_MASK ((1ull << PACK_SHIFT) - 1)

__device__ __forceinline__ bool row_passes_filters(const DevFilterSet &fs, uint64_t row) {
	bool ok = true;
	for (uint32_t i = 0; i < fs.n; i++) {
		const DevFilter &f = fs.f[i];
		const bool valid = !(f.valid && !f.valid[row]);
		if (f.op == POLR_CMP_IS_NULL) {
			ok = ok && !valid;
			continue;
		}
		if (f.op == POLR_CMP_IS_NOT_NULL) {
			ok = ok && valid;
			continue;
		}
		const uint64_t v = load_cell(as_global(f.data) + row * f.width, f.width, f.is_signed != 0);
		ok = ok && valid && int_cmp_holds(v, f.constant, f.op, f.is_signed != 0);
	}
	return ok;
}

// every comparison of every VARCHAR filter column holds for the row.  The validity byte comes first: the cell of a NULL
// row is never loaded, let alone its pointer followed (the reference leaves such cells as they were).
__device__ __forceinline__ bool row_passes_str(const DevStrSet &ss, uint64_t row) {
	bool ok = true;
	for (uint32_t c = 0; c < ss.n_cols; c++) {
		const DevStrCol &col = ss.col[c];
		if (col.valid && !as_global(col.valid)[row]) {
			ok = false; // NULL passes no comparison, <> included
		}
		if (ok) {
			const uint4 cell = load_global_x4(as_global((const uint32_t *)col.data) + row * 4);
			for (uint32_t i = col.first; i < col.first + col.n; i++) {
				const DevStrCmp &f = ss.cmp[i];
				ok = ok && polr_str_cmp_holds(polr_str_cmp3(cell.x, cell.y, cell.z, cell.w, f.c, ss.tails + f.tail_off), f.op);
			}
		}
	}
	return ok;
}

// The counting pass of every scan: one wave per vector (grid-stride), 64 rows per step.  `passes(row)` is the scan's row
// predicate; LIP is tested for the rows it keeps.  packed[v] = survivors of vector v with its non-empty flag; the ballot
// of every step goes to pass_bits, ceil(V / 64) words per vector, which the writing pass reads instead of evaluating again.
// All words of a vector are written, those beyond the table's last row as 0, so no word of an earlier scan is left in the
// range a scan uses.  (The kernels compute the wave ids: blockDim is read cheapest in the kernel function itself.)
template <class Pred>
__device__ __forceinline__ void tscan_count(uint32_t lane, uint64_t wave, uint64_t n_waves, const DevLipSet &lip, uint64_t n_rows,
                                            uint32_t V, uint64_t n_vec, unsigned long long *__restrict__ packed,
                                            unsigned long long *__restrict__ pass_bits, Pred passes) {
	const uint64_t words_per_vec = ((uint64_t)V + 63) >> 6;
	for (uint64_t v = wave; v < n_vec; v += n_waves) {
		const uint64_t begin = v * V;
		const uint64_t end = begin + V < n_rows ? begin + V : n_rows;
		uint64_t word = v * words_per_vec;
		uint32_t cnt = 0;
		for (uint64_t r0 = begin; r0 < begin + V; r0 += 64, word++) {
			const uint64_t row = r0 + lane;
			bool pass = row < end && passes(row);
			for (uint32_t i = 0; i < lip.n; i++) {
				pass = pass && lip_contains(lip.f[i], row);
			}
			const uint64_t m = __ballot(pass);
			cnt += (uint32_t)__popcll(m);
			if (lane == 0) {
				pass_bits[word] = m;
			}
		}
		if (lane == 0) {
			packed[v] = (unsigned long long)cnt | (cnt ? (1ull << PACK_SHIFT) : 0ull);
		}
	}
}
__global__ __launch_bounds__(256) void polr_tscan_count_kernel(DevFilterSet fs, DevLipSet lip, uint64_t n_rows, uint32_t V,
                                                              uint64_t n_vec, unsigned long long *__restrict__ packed,
                                                              unsigned long long *__restrict__ pass_bits) {
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
	tscan_count(lane, wave, n_waves, lip, n_rows, V, n_vec, packed, pass_bits,
	            [&](uint64_t row) { return row_passes_filters(fs, row); });
}
// ... with VARCHAR comparisons, evaluated for the rows the integer filters keep
__global__ __launch_bounds__(256) void polr_tscan_count_str_kernel(DevFilterSet fs, DevStrSet ss, DevLipSet lip, uint64_t n_rows,
                                                                  uint32_t V, uint64_t n_vec,
                                                                  unsigned long long *__restrict__ packed,
                                                                  unsigned long long *__restrict__ pass_bits) {
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
	tscan_count(lane, wave, n_waves, lip, n_rows, V, n_vec, packed, pass_bits,
	            [&](uint64_t row) { return row_passes_filters(fs, row) && row_passes_str(ss, row); });
}

// block sums of 1024 packed entries each
__global__ __launch_bounds__(1024) void polr_tscan_block_sums_kernel(const unsigned long long *__restrict__ packed,
                                                                    uint64_t n_vec,
                                                                    unsigned long long *__restrict__ sums) {
	__shared__ unsigned long long warp_sums[16];
	const uint64_t i = (uint64_t)blockIdx.x * 1024 + threadIdx.x;
	unsigned long long v = i < n_vec ? packed[i] : 0ull;
	for (int d = 32; d > 0; d >>= 1) {
		v += __shfl_down(v, d, 64);
	}
	if ((threadIdx.x & 63) == 0) {
		warp_sums[threadIdx.x >> 6] = v;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		unsigned long long s = 0;
		for (int w = 0; w < 16; w++) {
			s += warp_sums[w];
		}
		sums[blockIdx.x] = s;
	}
}

// one block: exclusive scan of the block sums in place; total -> totals[0] (tuples), totals[1] (chunks)
__global__ __launch_bounds__(1024) void polr_tscan_sums_kernel(unsigned long long *__restrict__ sums, uint64_t n_blocks,
                                                              unsigned long long *__restrict__ totals) {
	__shared__ unsigned long long warp_tot[16];
	__shared__ unsigned long long carry_s;
	if (threadIdx.x == 0) {
		carry_s = 0;
	}
	__syncthreads();
	for (uint64_t base = 0; base < n_blocks; base += 1024) {
		const uint64_t i = base + threadIdx.x;
		const unsigned long long mine = i < n_blocks ? sums[i] : 0ull;
		unsigned long long incl = mine;
		for (int d = 1; d < 64; d <<= 1) {
			const unsigned long long o = __shfl_up(incl, d, 64);
			if ((int)(threadIdx.x & 63) >= d) {
				incl += o;
			}
		}
		if ((threadIdx.x & 63) == 63) {
			warp_tot[threadIdx.x >> 6] = incl;
		}
		__syncthreads();
		unsigned long long before = carry_s;
		for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) {
			before += warp_tot[w];
		}
		if (i < n_blocks) {
			sums[i] = before + incl - mine;
		}
		__syncthreads();
		if (threadIdx.x == 1023) {
			carry_s = before + incl;
		}
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		totals[0] = carry_s & PACK_MASK;
		totals[1] = carry_s >> PACK_SHIFT;
	}
}

// exclusive prefix of every vector = block base + scan inside the block of 1024; in place
__global__ __launch_bounds__(1024) void polr_tscan_apply_kernel(unsigned long long *__restrict__ packed, uint64_t n_vec,
                                                               const unsigned long long *__restrict__ sums) {
	__shared__ unsigned long long warp_tot[16];
	const uint64_t i = (uint64_t)blockIdx.x * 1024 + threadIdx.x;
	const unsigned long long mine = i < n_vec ? packed[i] : 0ull;
	unsigned long long incl = mine;
	for (int d = 1; d < 64; d <<= 1) {
		const unsigned long long o = __shfl_up(incl, d, 64);
		if ((int)(threadIdx.x & 63) >= d) {
			incl += o;
		}
	}
	if ((threadIdx.x & 63) == 63) {
		warp_tot[threadIdx.x >> 6] = incl;
	}
	__syncthreads();
	unsigned long long before = sums[blockIdx.x];
	for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) {
		before += warp_tot[w];
	}
	if (i < n_vec) {
		// keep this vector's own non-empty flag in bit 63 (the write kernel needs it)
		packed[i] = (before + incl - mine) | ((mine >> PACK_SHIFT) ? (1ull << 63) : 0ull);
	}
}

// ---- expression filters (polr_pipeline_scan_filter_expr): what the reference evaluates in a PhysicalFilter behind the scan
// -- OR / NOT trees, IN lists, LIKE -- as a postfix program (lowered by polr_filter_plan.h).  The evaluator, fx_row_true, and
// the program's device form stand in polr_fx_device.h: the filter of a build side (polr_htfilter.hip) runs the same one.
__global__ __launch_bounds__(256) void polr_tscan_count_expr_kernel(DevFxProg px, DevLipSet lip, uint64_t n_rows, uint32_t V,
                                                                   uint64_t n_vec, unsigned long long *__restrict__ packed,
                                                                   unsigned long long *__restrict__ pass_bits) {
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
	tscan_count(lane, wave, n_waves, lip, n_rows, V, n_vec, packed, pass_bits, [&](uint64_t row) { return fx_row_true(px, row); });
}

// the writing pass of every scan, one wave per vector: ascending row ids of the survivors, read from the counting pass's
// bits, and the chunk boundary of every non-empty vector
__global__ __launch_bounds__(256) void polr_tscan_write_bits_kernel(const unsigned long long *__restrict__ pass_bits, uint64_t n_rows,
                                                                   uint32_t V, uint64_t n_vec,
                                                                   const unsigned long long *__restrict__ prefix,
                                                                   uint32_t *__restrict__ sel, uint64_t *__restrict__ chunk_offsets,
                                                                   const unsigned long long *__restrict__ totals) {
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
	const uint64_t words_per_vec = ((uint64_t)V + 63) >> 6;
	if (wave == 0 && lane == 0) {
		chunk_offsets[totals[1]] = totals[0]; // the end of the last chunk
	}
	for (uint64_t v = wave; v < n_vec; v += n_waves) {
		const unsigned long long pv = prefix[v];
		if (!(pv >> 63)) {
			continue; // no survivor: the scan skips the vector
		}
		uint64_t out = pv & PACK_MASK;
		const uint64_t chunk = (pv & ~(1ull << 63)) >> PACK_SHIFT;
		if (lane == 0) {
			chunk_offsets[chunk] = out;
		}
		const uint64_t begin = v * V;
		const uint64_t end = begin + V < n_rows ? begin + V : n_rows;
		uint64_t word = v * words_per_vec;
		for (uint64_t r0 = begin; r0 < end; r0 += 64, word++) {
			const uint64_t m = pass_bits[word];
			if ((m >> lane) & 1ull) {
				sel[out + lane_rank(m)] = (uint32_t)(r0 + lane);
			}
			out += (uint64_t)__popcll(m);
		}
	}
}

// the guard of a VARCHAR filter column whose cells were never rebased onto a device heap: its non-NULL cells longer than 12
// bytes -- their pointers are the host's.  Reads the validity byte and the length word of a cell, nothing else.
__global__ __launch_bounds__(256) void polr_tscan_count_long_kernel(const uint8_t *__restrict__ cells,
                                                                   const uint8_t *__restrict__ valid, uint64_t n_rows,
                                                                   unsigned long long *__restrict__ n_long) {
	unsigned long long mine = 0;
	for (uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n_rows; row += (uint64_t)gridDim.x * blockDim.x) {
		if (valid && !valid[row]) {
			continue;
		}
		mine += *(const uint32_t *)(cells + row * 16u) > 12u ? 1u : 0u;
	}
	mine = wave_sum64(mine);
	if ((threadIdx.x & 63u) == 0 && mine) {
		atomicAdd(n_long, mine);
	}
}

static int scan_filter_run(polr_pipeline *p, void *stream, const polr_scan_filter *filters, const polr_scan_filter_str *sfilters,
                           uint32_t n_filters, uint32_t lip_joins, uint32_t vector_size, uint64_t *n_selected,
                           uint64_t *n_chunks);

extern "C" {

int polr_pipeline_scan_filter(polr_pipeline *p, void *stream, const polr_scan_filter *filters, uint32_t n_filters,
                              uint32_t vector_size, uint64_t *n_selected, uint64_t *n_chunks) {
	return polr_pipeline_scan_filter_lip(p, stream, filters, n_filters, 0, vector_size, n_selected, n_chunks);
}

int polr_pipeline_scan_filter_lip(polr_pipeline *p, void *stream, const polr_scan_filter *filters, uint32_t n_filters,
                                  uint32_t lip_joins, uint32_t vector_size, uint64_t *n_selected, uint64_t *n_chunks) {
	POLR_ENTRY();
	if (!p || (!filters && n_filters)) {
		return POLR_E_INVALID;
	}
	return scan_filter_run(p, stream, filters, nullptr, n_filters, lip_joins, vector_size, n_selected, n_chunks);
}

int polr_pipeline_scan_filter_str(polr_pipeline *p, void *stream, const polr_scan_filter_str *filters, uint32_t n_filters,
                                  uint32_t lip_joins, uint32_t vector_size, uint64_t *n_selected, uint64_t *n_chunks) {
	POLR_ENTRY();
	if (!p || (!filters && n_filters)) {
		return POLR_E_INVALID;
	}
	return scan_filter_run(p, stream, nullptr, filters, n_filters, lip_joins, vector_size, n_selected, n_chunks);
}

} // extern "C"

// LIP: the joins whose filters are applied at the source, smallest index structure first (cheapest test first)
static int scan_lip_set(polr_pipeline *p, uint32_t lip_joins, DevLipSet &lip) {
	polr_ctx *ctx = p->ctx;
	memset(&lip, 0, sizeof(lip));
	{
		std::vector<uint32_t> js;
		for (uint32_t j = 0; j < p->k; j++) {
			if (!((lip_joins >> j) & 1u)) {
				continue;
			}
			if (p->hts[j]->n_keys != 1 || p->host_count.joins[j].key_src_join[0] >= 0) {
				POLR_FAIL(ctx, POLR_E_INVALID, "LIP: join %u is not keyed by one column of the source (physical_join.cpp:57-107)", j);
			}
			if (p->hts[j]->pack.packed) {
				POLR_FAIL(ctx, POLR_E_UNSUPPORTED, "LIP: join %u compares its key by value / NULL = NULL (packed form)", j);
			}
			js.push_back(j);
		}
		if (lip_joins >> p->k) {
			POLR_FAIL(ctx, POLR_E_INVALID, "LIP: join mask names a join beyond the %u of the pipeline", p->k);
		}
		std::sort(js.begin(), js.end(), [&](uint32_t a, uint32_t b) { return p->hts[a]->device_bytes < p->hts[b]->device_bytes; });
		for (uint32_t j : js) {
			// (the build side itself says what its index is like; DevJoin keeps where the caller's descriptor reads the key)
			const polr_ht *ht = p->hts[j];
			const OwnedCol &c = p->probe_cols[p->host_count.joins[j].key_src_col[0]];
			DevLip &f = lip.f[lip.n++];
			f.key_data = c.data;
			f.key_valid = c.valid;
			f.key_width = c.width;
			f.key_signed = ht->key_signed ? 1 : 0;
			f.kind = ht->kind;
			f.table = ht->table;
			f.mask = ht_mask(ht);
			f.min_value = ht->min_value;
			f.range = ht->range;
			f.sentinel_count = ht->sentinel_count;
		}
	}
	return POLR_OK;
}

// A VARCHAR filter column the library uploaded whose heap never came may hold inline strings only (see scan_filter_run)
static int scan_check_heap(polr_pipeline *p, hipStream_t st, uint32_t col) {
	polr_ctx *ctx = p->ctx;
	const OwnedCol &c = p->probe_cols[col];
	if (c.strings_rebased || !c.owned() || p->n_probe_rows == 0) {
		return POLR_OK;
	}
	DevBuf<unsigned long long> n_long;
	unsigned long long h_long = 0;
	HIPCHK(ctx, n_long.alloc(1));
	HIPCHK(ctx, hipMemsetAsync(n_long, 0, 8, st));
	const uint32_t grid = (uint32_t)std::min<uint64_t>((p->n_probe_rows + 255) / 256, (uint64_t)ctx->n_cus * 8);
	hipLaunchKernelGGL(polr_tscan_count_long_kernel, dim3(grid), dim3(256), 0, st, (const uint8_t *)c.data,
	                   (const uint8_t *)c.valid, p->n_probe_rows, n_long.get());
	HIPCHK(ctx, hipMemcpyAsync(&h_long, n_long, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	if (h_long) {
		POLR_FAIL(ctx, POLR_E_INVALID,
		          "filter column %u: %llu rows hold strings longer than 12 bytes, but the column's heap was never put on the "
		          "device (polr_pipeline_set_probe_heaps)",
		          col, h_long);
	}
	return POLR_OK;
}

// the vector size and the table fit the scan: what every entry point checks before it looks at its filters
static int scan_check_shape(polr_pipeline *p, uint32_t vector_size) {
	polr_ctx *ctx = p->ctx;
	if (vector_size < 2 || vector_size > 65536) {
		POLR_FAIL(ctx, POLR_E_INVALID, "vector size %u out of range", vector_size);
	}
	if (p->n_probe_rows >= 0xFFFFFFF0ull) {
		POLR_FAIL(ctx, POLR_E_UNSUPPORTED, "source partition too large for 32-bit row ids");
	}
	return POLR_OK;
}

// the scan's scratch and result buffers, grown to the table, the vector count and the pass-bit words (see scan_run)
static int scan_buffers(polr_pipeline *p, uint64_t n_rows, uint64_t n_vec, uint64_t n_blocks, uint64_t n_words) {
	polr_ctx *ctx = p->ctx;
	const uint32_t *old_sel = p->scan_sel;
	hipError_t e = p->scan_packed.ensure(std::max<uint64_t>(n_vec, 1));
	e = e == hipSuccess ? p->scan_sums.ensure(std::max<uint64_t>(n_blocks, 1)) : e;
	e = e == hipSuccess ? p->scan_totals.ensure(2) : e;
	e = e == hipSuccess ? p->scan_pass_bits.ensure(std::max<uint64_t>(n_words, 1)) : e;
	e = e == hipSuccess ? p->scan_sel.ensure(std::max<uint64_t>(n_rows, 1)) : e;
	e = e == hipSuccess ? p->scan_offsets_dev.ensure(n_vec + 1) : e;
	if (p->sel_dev && p->sel_dev == old_sel && old_sel != p->scan_sel) {
		p->sel_dev = nullptr; // (the selection in use was the scan result that just went)
	}
	if (e != hipSuccess) {
		POLR_FAIL(ctx, POLR_E_HIP, "scan filter buffers: %s", hipGetErrorString(e));
	}
	return POLR_OK;
}

static int scan_install(polr_pipeline *p, uint32_t vector_size, const uint64_t *h_tot, uint64_t *n_selected, uint64_t *n_chunks) {
	polr_ctx *ctx = p->ctx;
	uint32_t *sel = p->scan_sel;
	// install: the selection is the pipeline's source now (the buffers stay the pipeline's scan buffers)
	p->sel_upload.reset();
	p->sel_dev = sel;
	p->n_tuples = h_tot[0];
	p->scan_valid = true;
	p->scan_generation++;
	p->scan_n_chunks = h_tot[1];
	p->scan_vector_size = vector_size;
	p->host_mat.sel = p->sel_dev;
	p->host_mat.n_tuples = p->n_tuples;
	p->host_count.sel = p->sel_dev;
	p->host_count.n_tuples = p->n_tuples;
	HIPCHK(ctx, hipMemcpy(p->dev_mat, &p->host_mat, sizeof(DevPipeline), hipMemcpyHostToDevice));
	HIPCHK(ctx, hipMemcpy(p->dev_count, &p->host_count, sizeof(DevPipeline), hipMemcpyHostToDevice));
	if (n_selected) {
		*n_selected = h_tot[0];
	}
	if (n_chunks) {
		*n_chunks = h_tot[1];
	}
	return POLR_OK;
}

// The scan behind all four entry points, from the settling of a re-scan to the installed result.  The caller has checked
// and lowered its filters (and uploaded what they need); `enqueue_count(grid, lip, n_rows, n_vec, packed, pass_bits)` enqueues
// its counting kernel on `st`.
template <class EnqueueCount>
static int scan_run(polr_pipeline *p, hipStream_t st, uint32_t vector_size, const DevLipSet &lip, uint64_t *n_selected,
                    uint64_t *n_chunks, EnqueueCount enqueue_count) {
	polr_ctx *ctx = p->ctx;
	if (p->scan_valid) {
		// A re-scan rewrites the selection, the chunk boundaries and the device copies of the pipeline in place, and runs
		// of the previous scan may still be in flight on their multiplexers' streams (passes are enqueued without a
		// host synchronisation): settle the device first.  (The first scan of a pipeline has nothing to wait for.)
		HIPCHK(ctx, hipDeviceSynchronize());
	}
	const uint64_t n_rows = p->n_probe_rows;
	const uint64_t n_vec = (n_rows + vector_size - 1) / vector_size;
	const uint64_t n_blocks = (n_vec + 1023) / 1024;
	if (n_vec >= (1ull << 23)) {
		POLR_FAIL(ctx, POLR_E_UNSUPPORTED, "more than 2^23 scan vectors per partition");
	}
	// Scratch and result buffers belong to the pipeline and are sized for the worst case (every row survives, every
	// vector is a chunk; one pass-bit word per 64-row step of a vector), so the whole scan is enqueued without a host
	// round trip in the middle; one synchronisation at the end reads the two totals.
	if (int rc = scan_buffers(p, n_rows, n_vec, n_blocks, n_vec * (((uint64_t)vector_size + 63) / 64))) {
		return rc;
	}
	unsigned long long *packed = p->scan_packed, *sums = p->scan_sums, *totals = p->scan_totals, *bits = p->scan_pass_bits;
	uint32_t *sel = p->scan_sel;
	uint64_t *offs = p->scan_offsets_dev;
	uint64_t h_tot[2] = {0, 0};
	hipError_t e = hipSuccess;
	if (n_vec) {
		const uint32_t waves_per_block = 4;
		const uint32_t grid = (uint32_t)std::min<uint64_t>((n_vec + waves_per_block - 1) / waves_per_block,
		                                                   (uint64_t)ctx->n_cus * 8);
		enqueue_count(grid, lip, n_rows, n_vec, packed, bits);
		hipLaunchKernelGGL(polr_tscan_block_sums_kernel, dim3((uint32_t)n_blocks), dim3(1024), 0, st, packed, n_vec, sums);
		hipLaunchKernelGGL(polr_tscan_sums_kernel, dim3(1), dim3(1024), 0, st, sums, n_blocks, totals);
		hipLaunchKernelGGL(polr_tscan_apply_kernel, dim3((uint32_t)n_blocks), dim3(1024), 0, st, packed, n_vec, sums);
		hipLaunchKernelGGL(polr_tscan_write_bits_kernel, dim3(grid), dim3(256), 0, st, (const unsigned long long *)bits, n_rows,
		                   vector_size, n_vec, (const unsigned long long *)packed, sel, offs, (const unsigned long long *)totals);
		e = hipMemcpyAsync(h_tot, totals, 16, hipMemcpyDeviceToHost, st);
		e = e == hipSuccess ? hipStreamSynchronize(st) : e;
	} else {
		e = hipMemsetAsync(offs, 0, 8, st);
		e = e == hipSuccess ? hipStreamSynchronize(st) : e;
	}
	if (e != hipSuccess) {
		POLR_FAIL(ctx, POLR_E_HIP, "scan filter failed: %s", hipGetErrorString(e));
	}
	return scan_install(p, vector_size, h_tot, n_selected, n_chunks);
}

// The integer and VARCHAR entry points: filters checked and lowered, then scan_run.  `filters`:
// polr_pipeline_scan_filter[_lip], every filter an integer one whatever the column's width; `sfilters`:
// polr_pipeline_scan_filter_str, where a comparison on a 16-byte column is a VARCHAR one.
static int scan_filter_run(polr_pipeline *p, void *stream, const polr_scan_filter *filters, const polr_scan_filter_str *sfilters,
                           uint32_t n_filters, uint32_t lip_joins, uint32_t vector_size, uint64_t *n_selected,
                           uint64_t *n_chunks) {
	polr_ctx *ctx = p->ctx;
	if (n_filters > POLR_MAX_FILTERS) {
		POLR_FAIL(ctx, POLR_E_UNSUPPORTED, "at most %d pushed-down filters", POLR_MAX_FILTERS);
	}
	if (int rc = scan_check_shape(p, vector_size)) {
		return rc;
	}
	DevFilterSet fs;
	memset(&fs, 0, sizeof(fs));
	DevStrSet ss;
	memset(&ss, 0, sizeof(ss));
	std::vector<uint8_t> tails; // the VARCHAR constants' bytes beyond 12
	uint32_t str_col[POLR_MAX_FILTERS];      // probe column of ss.col[c]
	std::vector<uint32_t> str_of[POLR_MAX_FILTERS]; // its comparisons (indices into sfilters)
	for (uint32_t i = 0; i < n_filters; i++) {
		polr_scan_filter f;
		if (sfilters) {
			f.col = sfilters[i].col;
			f.op = sfilters[i].op;
			f.constant = sfilters[i].constant;
		} else {
			f = filters[i];
		}
		if (f.col >= p->n_probe_cols) {
			POLR_FAIL(ctx, POLR_E_INVALID, "filter %u: column %u out of range", i, f.col);
		}
		if (f.op > POLR_CMP_IS_NOT_NULL) {
			POLR_FAIL(ctx, POLR_E_INVALID, "filter %u: unknown comparison %u", i, f.op);
		}
		const OwnedCol &c = p->probe_cols[f.col];
		if (sfilters) {
			const polr_scan_filter_str &sf = sfilters[i];
			if (!sf.str && sf.str_len) {
				POLR_FAIL(ctx, POLR_E_INVALID, "filter %u: a string constant of %llu bytes without its bytes", i,
				          (unsigned long long)sf.str_len);
			}
			if (sf.str && c.width != 16) {
				POLR_FAIL(ctx, POLR_E_INVALID, "filter %u: a string constant against column %u, which is %u bytes wide", i, f.col, c.width);
			}
			if (sf.str_len > POLR_MAX_FILTER_STRING) {
				POLR_FAIL(ctx, POLR_E_UNSUPPORTED, "filter %u: a string constant of %llu bytes (at most %d)", i,
				          (unsigned long long)sf.str_len, POLR_MAX_FILTER_STRING);
			}
			if (c.width == 16 && f.op <= POLR_CMP_GE) {
				// a VARCHAR comparison: grouped by column, so that the cell is loaded once for all its constants
				uint32_t g = 0;
				while (g < ss.n_cols && str_col[g] != f.col) {
					g++;
				}
				if (g == ss.n_cols) {
					str_col[ss.n_cols++] = f.col;
				}
				str_of[g].push_back(i);
				continue;
			}
		}
		// (IS [NOT] NULL reads the validity only, whatever the column holds)
		const bool is_signed = (c.flags & 1u) != 0;
		if (!is_signed && f.constant < 0 && f.op <= POLR_CMP_GE) {
			POLR_FAIL(ctx, POLR_E_INVALID, "filter %u: negative constant against an unsigned column", i);
		}
		DevFilter &d = fs.f[fs.n++];
		d.data = c.data;
		d.valid = c.valid;
		d.width = c.width;
		d.is_signed = is_signed ? 1u : 0u;
		d.op = f.op;
		d.constant = f.constant;
	}
	for (uint32_t g = 0, at = 0; g < ss.n_cols; g++) {
		const OwnedCol &c = p->probe_cols[str_col[g]];
		ss.col[g].data = c.data;
		ss.col[g].valid = c.valid;
		ss.col[g].first = at;
		ss.col[g].n = (uint32_t)str_of[g].size();
		for (uint32_t i : str_of[g]) {
			const polr_scan_filter_str &sf = sfilters[i];
			DevStrCmp &d = ss.cmp[at++];
			d.c = polr_str_const_make((const uint8_t *)sf.str, sf.str_len);
			d.op = sf.op;
			d.tail_off = (uint32_t)tails.size();
			if (sf.str_len > 12) {
				tails.insert(tails.end(), (const uint8_t *)sf.str + 12, (const uint8_t *)sf.str + sf.str_len);
			}
		}
	}
	DevLipSet lip;
	if (int rc = scan_lip_set(p, lip_joins, lip)) {
		return rc;
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	// A VARCHAR filter column the library uploaded whose heap never came (polr_pipeline_set_probe_heaps) may hold inline
	// strings only: counted from the length words before any kernel that follows a pointer is enqueued.  (A
	// POLR_COL_DEVICE column points into HBM by contract.)
	for (uint32_t g = 0; g < ss.n_cols; g++) {
		if (int rc = scan_check_heap(p, st, str_col[g])) {
			return rc;
		}
	}
	if (!tails.empty()) {
		HIPCHK(ctx, p->scan_str_tails.ensure((size_t)POLR_MAX_FILTERS * POLR_MAX_FILTER_STRING));
		// (no scan kernel is in flight: every scan call ends with a synchronisation of its stream)
		HIPCHK(ctx, hipMemcpy(p->scan_str_tails, tails.data(), tails.size(), hipMemcpyHostToDevice));
	}
	ss.tails = p->scan_str_tails;
	return scan_run(p, st, vector_size, lip, n_selected, n_chunks,
	                [&](uint32_t grid, const DevLipSet &l, uint64_t n_rows, uint64_t n_vec, unsigned long long *packed, unsigned long long *bits) {
		                if (ss.n_cols) {
			                hipLaunchKernelGGL(polr_tscan_count_str_kernel, dim3(grid), dim3(256), 0, st, fs, ss, l, n_rows, vector_size,
			                                   n_vec, packed, bits);
		                } else {
			                hipLaunchKernelGGL(polr_tscan_count_kernel, dim3(grid), dim3(256), 0, st, fs, l, n_rows, vector_size, n_vec,
			                                   packed, bits);
		                }
	                });
}

// polr_pipeline_scan_filter_expr: the program checked and lowered on the host (polr_filter_plan.h), uploaded into the
// pipeline's program buffer, then scan_run
static int scan_filter_expr_run(polr_pipeline *p, void *stream, const polr_filter_node *nodes, uint32_t n_nodes,
                                const polr_filter_value *values, uint32_t n_values, uint32_t lip_joins, uint32_t vector_size,
                                uint64_t *n_selected, uint64_t *n_chunks) {
	polr_ctx *ctx = p->ctx;
	if (int rc = scan_check_shape(p, vector_size)) {
		return rc;
	}
	std::vector<PolrFilterColumn> cols(p->n_probe_cols);
	for (uint32_t c = 0; c < p->n_probe_cols; c++) {
		cols[c].width = p->probe_cols[c].width;
		cols[c].is_signed = p->probe_cols[c].flags & 1u;
	}
	PolrFilterPlan pl;
	if (int rc = polr_filter_plan(nodes, n_nodes, values, n_values, cols.data(), p->n_probe_cols, pl)) {
		POLR_FAIL(ctx, rc, "filter expression: %s", pl.err);
	}
	DevLipSet lip;
	if (int rc = scan_lip_set(p, lip_joins, lip)) {
		return rc;
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	// (the heaps: as scan_filter_run -- only columns whose cells some leaf reads)
	for (uint32_t g = 0; g < pl.n_cols; g++) {
		if (pl.cols[g].needs_cell && cols[pl.cols[g].col].width == 16) {
			if (int rc = scan_check_heap(p, st, pl.cols[g].col)) {
				return rc;
			}
		}
	}
	// the program buffer (polr_fx_device.h lays it out)
	PolrFxBlob blob;
	polr_fx_blob_make(pl, blob);
	HIPCHK(ctx, p->scan_expr_prog.ensure(std::max<size_t>(blob.bytes.size(), 8192)));
	// (no scan kernel is in flight: every scan call ends with a synchronisation of its stream)
	HIPCHK(ctx, hipMemcpy(p->scan_expr_prog, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice));
	DevFxProg px;
	polr_fx_prog_make(pl, blob, p->scan_expr_prog.get(), [&](uint32_t c) -> const OwnedCol & { return p->probe_cols[c]; }, px);
	return scan_run(p, st, vector_size, lip, n_selected, n_chunks,
	                [&](uint32_t grid, const DevLipSet &l, uint64_t n_rows, uint64_t n_vec, unsigned long long *packed, unsigned long long *bits) {
		                hipLaunchKernelGGL(polr_tscan_count_expr_kernel, dim3(grid), dim3(256), 0, st, px, l, n_rows, vector_size, n_vec,
		                                   packed, bits);
	                });
}

extern "C" {

int polr_pipeline_scan_filter_expr(polr_pipeline *p, void *stream, const polr_filter_node *nodes, uint32_t n_nodes,
                                   const polr_filter_value *values, uint32_t n_values, uint32_t lip_joins,
                                   uint32_t vector_size, uint64_t *n_selected, uint64_t *n_chunks) {
	POLR_ENTRY();
	if (!p) {
		return POLR_E_INVALID;
	}
	return scan_filter_expr_run(p, stream, nodes, n_nodes, values, n_values, lip_joins, vector_size, n_selected, n_chunks);
}


int polr_pipeline_fetch_scan(polr_pipeline *p, uint32_t *sel, uint64_t *chunk_offsets) {
	POLR_ENTRY();
	if (!p) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = p->ctx;
	if (!p->scan_valid) {
		POLR_FAIL(ctx, POLR_E_INVALID, "no scan result: call polr_pipeline_scan_filter first");
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (sel && p->n_tuples) {
		HIPCHK(ctx, hipMemcpy(sel, p->sel_dev, p->n_tuples * 4, hipMemcpyDeviceToHost));
	}
	if (chunk_offsets) {
		HIPCHK(ctx, hipMemcpy(chunk_offsets, p->scan_offsets_dev, (p->scan_n_chunks + 1) * 8, hipMemcpyDeviceToHost));
	}
	return POLR_OK;
}

} // extern "C"
