// duckdb-polr_amd/csrc/polr_htsemi.hip -- polr_ht_semi_filter: the rows of an un-finalized build side thinned by SEMI / ANTI
// joins against finalized tables and compacted on the device (the SEMI / ANTI / MARK hash joins inside a build subtree,
// polar_enumeration_algo.cpp:192-205; ScanStructure::NextSemiJoin / NextAntiJoin, join_hashtable.cpp:589-627) -- LIP for
// build sides.  Contract: include/polr_hip.h; the request checked and laid out: polr_htsemi_plan.h.
//
// The passes of polr_ht_filter with another counting kernel:
//   counting    one wave per tile of 1024 rows; a lane has HTS_R rows of the tile at a time, one of each of HTS_R consecutive
//               64-row words.  Per filter (up to four, cheapest first) it loads the validity bytes and the key cells of its
//               HTS_R rows together, forms the keys, and probes `by`'s index for the rows still alive -- bit table, unique-key
//               or run hash table -- with the first slot-group loads of its HTS_R rows issued together and one 32-byte slot
//               group per further round trip (perfect_index, s8_group_step, s16_begin_probe / s16_group_step of
//               polr_device.h).  The key arithmetic is one for the plain and the packed form (polr_htsemi_plan.h).  The
//               ballots are the pass-bit words, their popcounts the tile's count.  The filter descriptors travel by value
//               (kernel arguments: scalar loads).
//   prefix, compaction   polr_chunk_prefix_kernel and polr_htfilter_compact_kernel as polr_ht_filter launches them; a table
//               filtered before has its row list compacted as one more 4-byte column, which makes the composed list.
// Every access is global_load / global_store: no FLAT instruction, no scratch.
// Algorithmic bytes per table row: the widths of the key columns plus their validity bytes, once per filter that still
// tests the row; one slot group (32 bytes) or one bit-table word (4 bytes) per probe; 2 x 1/8 for the pass bit; per kept
// row what polr_ht_filter's compaction moves.
//
// HTS_R = 1 is what ships.  Several rows per lane (HTS_R = 4, the compaction kernel's shape: four independent load chains per
// lane) were measured against it on the same input -- tools/bench_ht_semi.py, 30 M rows against 1 M keys, whole calls: against
// a unique-key hash table 1.007 ms with four rows and 0.945 ms with one (SEMI; ANTI 1.053 / 1.010), a run hash table 1.013 /
// 0.990 (ANTI 1.066 / 1.063), two filters in one call 0.833 / 0.778; only against the 250 KB bit table of a perfect `by` were
// four rows ahead, 0.605 / 0.636 (ANTI 0.638 / 0.656); two rows lay between the two everywhere.  With one row a wave needs
// 30 VGPRs and all eight waves of a SIMD are resident, with four it needs 100 and five are: the rows in flight per SIMD grow
// less than the shape suggests, and 30 M probes into 16 or 32 MB of slots are presumably bound by the lines they move, not
// by the latency of one (no counter was collected).  (profiles/README.md, "Semi-join filtered build sides"; `make htsemi-r4` builds the other shape.)
// gfx950, the code object's metadata: counting 30 VGPRs / 80 SGPRs / no LDS with HTS_R = 1 (100 / 91 with HTS_R = 4); no
// scratch and no spills in either.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "polr_htsemi_plan.h"
#include "polr_internal.h"

#ifndef POLR_HTSEMI_R
#define POLR_HTSEMI_R 1u // rows a lane serves at a time (4: four independent load chains per lane, the shape it was measured against)
#endif
#define HTS_R POLR_HTSEMI_R
static_assert(POLR_HTFILTER_TILE_WORDS % HTS_R == 0, "a tile is a whole number of steps");

struct HtsKey { // one key column of a filter (PolrHtSemiKey with the column's addresses)
	const uint8_t *data, *valid;
	int64_t min;
	uint64_t range;
	uint32_t width, sx, shift, null_eq;
};
struct HtsFilter {
	const void *table; // S8: uint2[capacity]; S16: uint4[capacity]; perfect: uint32 bit words
	uint64_t mask;
	int64_t min_value;
	uint64_t range;
	uint32_t kind, key_signed, sentinel_count, n_keys, anti, pad;
	HtsKey key[POLR_NKEYS];
};
struct HtsSet {
	HtsFilter f[POLR_MAX_SEMI_FILTERS];
	uint32_t n, pad;
};

// HTS_R cells of one key column folded into the keys: the loads first, then the arithmetic (polr_htsemi_plan.h)
template <class T, class S>
__device__ __forceinline__ void hts_fold(const HtsKey &k, const uint64_t (&at)[HTS_R], uint64_t (&key)[HTS_R], bool (&valid)[HTS_R]) {
	const POLR_GLOBAL uint8_t *kv = as_global(k.valid);
	const POLR_GLOBAL T *kd = (const POLR_GLOBAL T *)as_global(k.data);
	uint8_t vb[HTS_R];
	T cell[HTS_R];
#pragma unroll
	for (uint32_t r = 0; r < HTS_R; r++) {
		vb[r] = kv ? kv[at[r]] : (uint8_t)1;
	}
#pragma unroll
	for (uint32_t r = 0; r < HTS_R; r++) {
		cell[r] = kd[at[r]];
	}
#pragma unroll
	for (uint32_t r = 0; r < HTS_R; r++) {
		const uint64_t v = k.sx ? (uint64_t)(int64_t)(S)cell[r] : (uint64_t)cell[r];
		uint64_t off = v - (uint64_t)k.min;
		if (!vb[r]) {
			if (k.null_eq) {
				off = k.range + 1u; // IS NOT DISTINCT FROM: NULL is a key value of its own
			} else {
				valid[r] = false;
			}
		} else if (off > k.range) {
			valid[r] = false;
		}
		key[r] |= off << k.shift;
	}
}

// does filter f keep the lane's rows?  at[]: the rows to read (inside the table also for a row that is not alive)
__device__ __forceinline__ void hts_filter(const HtsFilter &f, const uint64_t (&at)[HTS_R], bool (&alive)[HTS_R]) {
	uint64_t key[HTS_R];
	bool valid[HTS_R], hit[HTS_R];
#pragma unroll
	for (uint32_t r = 0; r < HTS_R; r++) {
		key[r] = 0;
		valid[r] = alive[r];
		hit[r] = false;
	}
	for (uint32_t c = 0; c < f.n_keys; c++) {
		const HtsKey &k = f.key[c];
		switch (k.width) {
		case 1:
			hts_fold<uint8_t, int8_t>(k, at, key, valid);
			break;
		case 2:
			hts_fold<uint16_t, int16_t>(k, at, key, valid);
			break;
		case 4:
			hts_fold<uint32_t, int32_t>(k, at, key, valid);
			break;
		default:
			hts_fold<uint64_t, int64_t>(k, at, key, valid);
			break;
		}
	}
	if (f.kind == KIND_PERFECT) {
		const POLR_GLOBAL uint32_t *bits = as_global((const uint32_t *)f.table);
		uint64_t idx[HTS_R];
		uint32_t word[HTS_R];
#pragma unroll
		for (uint32_t r = 0; r < HTS_R; r++) {
			valid[r] = perfect_index(key[r], f.key_signed != 0, f.min_value, f.range, idx[r]) && valid[r];
		}
#pragma unroll
		for (uint32_t r = 0; r < HTS_R; r++) {
			word[r] = 0;
			if (valid[r]) {
				word[r] = bits[idx[r] >> 5];
			}
		}
#pragma unroll
		for (uint32_t r = 0; r < HTS_R; r++) {
			hit[r] = ((word[r] >> (idx[r] & 31)) & 1u) != 0;
		}
	} else {
		// one aligned 32-byte slot group per round trip: four {key32, row} slots or two {key64, start, count} slots
		const POLR_GLOBAL uint32_t *tab = as_global((const uint32_t *)f.table);
		const bool s8 = f.kind == KIND_S8;
		const uint64_t group_mask = f.mask >> (s8 ? 2 : 1);
		uint64_t group[HTS_R];
		uint32_t first[HTS_R], start[HTS_R], count[HTS_R];
		bool searching[HTS_R], any = false;
#pragma unroll
		for (uint32_t r = 0; r < HTS_R; r++) {
			start[r] = count[r] = 0;
			if (s8) {
				key[r] = (uint32_t)key[r];
				searching[r] = valid[r];
			} else {
				s16_begin_probe(key[r], valid[r], 0, f.sentinel_count, searching[r], start[r], count[r]);
			}
			const uint64_t h = polr_murmurhash64(key[r]) & f.mask;
			group[r] = h >> (s8 ? 2 : 1);
			first[r] = (uint32_t)h & (s8 ? 3u : 1u);
			any = any || searching[r];
		}
		while (any) {
			uint4 a[HTS_R], b[HTS_R];
#pragma unroll
			for (uint32_t r = 0; r < HTS_R; r++) {
				a[r] = b[r] = make_uint4(0, 0, 0, 0);
				if (searching[r]) {
					a[r] = load_global_x4(tab + group[r] * 8u);
					b[r] = load_global_x4(tab + group[r] * 8u + 4u);
				}
			}
			any = false;
#pragma unroll
			for (uint32_t r = 0; r < HTS_R; r++) {
				if (searching[r]) {
					if (s8) {
						s8_group_step(a[r], b[r], first[r], (uint32_t)key[r], searching[r], hit[r], start[r]);
					} else {
						s16_group_step(a[r], b[r], first[r], key[r], searching[r], start[r], count[r]);
					}
					first[r] = 0;
					group[r] = (group[r] + 1) & group_mask;
				}
				any = any || searching[r];
			}
		}
		if (!s8) {
#pragma unroll
			for (uint32_t r = 0; r < HTS_R; r++) {
				hit[r] = count[r] != 0; // (a key that repeats counts once; the all-ones key: the side entry's count)
			}
		}
	}
#pragma unroll
	for (uint32_t r = 0; r < HTS_R; r++) {
		alive[r] = alive[r] && (f.anti ? !hit[r] : hit[r]);
	}
}

// the counting pass: pass_bits[n_tiles * 16] (rows behind the table's last: 0), tile_count[n_tiles]; n_rows > 0
__global__ __launch_bounds__(256) void polr_htsemi_count_kernel(HtsSet fs, uint64_t n_rows, uint64_t n_tiles,
                                                                unsigned long long *__restrict__ pass_bits,
                                                                uint32_t *__restrict__ tile_count) {
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
	for (uint64_t tile = wave; tile < n_tiles; tile += n_waves) {
		const uint64_t begin = tile * POLR_HTFILTER_TILE;
		uint32_t cnt = 0;
		for (uint32_t w0 = 0; w0 < POLR_HTFILTER_TILE_WORDS; w0 += HTS_R) {
			uint64_t at[HTS_R];
			bool alive[HTS_R];
#pragma unroll
			for (uint32_t r = 0; r < HTS_R; r++) {
				const uint64_t row = begin + (uint64_t)(w0 + r) * 64u + lane;
				alive[r] = row < n_rows;
				at[r] = alive[r] ? row : n_rows - 1; // (the key loads are not predicated: they stay inside the columns)
			}
			for (uint32_t i = 0; i < fs.n; i++) {
				hts_filter(fs.f[i], at, alive);
			}
#pragma unroll
			for (uint32_t r = 0; r < HTS_R; r++) {
				const uint64_t m = __ballot(alive[r]);
				cnt += (uint32_t)__popcll(m);
				if (lane == 0) {
					as_global(pass_bits)[tile * POLR_HTFILTER_TILE_WORDS + w0 + r] = m;
				}
			}
		}
		if (lane == 0) {
			as_global(tile_count)[tile] = cnt;
		}
	}
}

static OwnedCol &hts_col(polr_ht *ht, uint32_t c) {
	uint32_t idx;
	return polr_htfilter_col(c, ht->n_keys, idx) ? ht->keys[idx] : ht->payload[idx];
}

extern "C" int polr_ht_semi_filter(polr_ht *ht, void *stream, const polr_semi_filter *filters, uint32_t n_filters,
                                   uint64_t *n_kept) {
	POLR_ENTRY();
	if (!ht) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = ht->ctx;
	// refusals before anything is enqueued
	PolrHtSemiRequest rq = {};
	rq.has_ht = true;
	rq.finalized = ht->kind != KIND_NONE;
	rq.filtered = ht->filtered;
	rq.has_dict = !ht->dicts.empty();
	rq.dict_col = rq.has_dict ? ht->dicts[0].src_col : 0;
	rq.n_keys = ht->n_keys;
	rq.n_payload = ht->n_payload;
	rq.n_rows = ht->n_rows_in;
	rq.filters = filters;
	rq.n_filters = n_filters;
	std::vector<PolrHtSemiBy> bys(filters && n_filters <= POLR_MAX_SEMI_FILTERS ? n_filters : 0);
	for (uint32_t i = 0; i < bys.size(); i++) {
		const polr_ht *by = filters[i].by;
		PolrHtSemiBy &b = bys[i];
		b = PolrHtSemiBy();
		if (!by) {
			continue;
		}
		b.has_by = true;
		b.finalized = by->kind != KIND_NONE;
		b.is_ht = by == ht;
		b.same_place = by->ctx == ctx;
		b.kind = by->kind;
		b.n_keys = by->n_keys;
		for (uint32_t c = 0; c < by->n_keys && c < POLR_NKEYS; c++) {
			b.key_width[c] = by->keys[c].width;
			b.key_flags[c] = by->key_flags[c];
		}
		b.key_signed = by->key_signed ? 1 : 0;
		b.pack = by->pack;
		b.device_bytes = by->device_bytes;
	}
	rq.by = bys.data();
	const uint32_t n_cols = ht->n_keys + ht->n_payload;
	std::vector<PolrHtFilterColumn> shapes(n_cols);
	for (uint32_t c = 0; c < n_cols; c++) {
		const OwnedCol &col = hts_col(ht, c);
		shapes[c] = PolrHtFilterColumn{col.width, col.flags & POLR_COL_SIGNED, col.valid != nullptr, col.owned(), col.strings_rebased};
	}
	PolrHtSemiPlan plan;
	POLR_TRY_PLAN(ctx, plan, polr_htsemi_plan(rq, shapes.data(), plan));
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	if (st != ctx->stream) {
		// (the columns were uploaded, and the `by` tables built, on the context's stream unless the caller ordered otherwise)
		HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	}
	const uint64_t n = ht->n_rows_in;
	const PolrHtFilterPlan &sc = plan.scratch;
	DevBuf<uint8_t> scratch;
	HIPCHK(ctx, scratch.alloc(sc.scratch_bytes));
	uint64_t *total = (uint64_t *)(scratch.get() + sc.total_off);
	unsigned long long *bits = (unsigned long long *)(scratch.get() + sc.bits_off);
	uint64_t *tile_base = (uint64_t *)(scratch.get() + sc.base_off);
	uint32_t *tile_count = (uint32_t *)(scratch.get() + sc.count_off);
	// the counting pass, the tiles' first output rows, the total
	uint64_t kept = 0;
	if (n) {
		HtsSet fs;
		memset(&fs, 0, sizeof(fs));
		fs.n = plan.n_filters;
		for (uint32_t i = 0; i < plan.n_filters; i++) {
			const uint32_t src = plan.order[i];
			const polr_ht *by = filters[src].by;
			const PolrHtSemiFilter &pf = plan.f[src];
			HtsFilter &f = fs.f[i];
			f.table = by->table;
			f.mask = ht_mask(by);
			f.min_value = by->min_value;
			f.range = by->range;
			f.kind = by->kind;
			f.key_signed = by->key_signed ? 1 : 0;
			f.sentinel_count = by->sentinel_count;
			f.n_keys = pf.n_keys;
			f.anti = pf.anti;
			for (uint32_t c = 0; c < pf.n_keys; c++) {
				const OwnedCol &col = hts_col(ht, pf.key[c].col);
				f.key[c] = HtsKey{col.data, col.valid, pf.key[c].min, pf.key[c].range, pf.key[c].width, pf.key[c].sx,
				                  pf.key[c].shift, pf.key[c].null_eq};
			}
		}
		const uint32_t grid = (uint32_t)std::min<uint64_t>((sc.n_tiles + 3) / 4, (uint64_t)ctx->n_cus * 8);
		hipLaunchKernelGGL(polr_htsemi_count_kernel, dim3(grid), dim3(256), 0, st, fs, n, sc.n_tiles, bits, tile_count);
		polr_launch_chunk_prefix(st, (const uint32_t *)tile_count, (uint32_t)sc.n_tiles, tile_base, total);
		HIPCHK(ctx, hipMemcpyAsync(&kept, total, 8, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
	}
	// everything the table will hold, before the first kernel that writes into it
	PolrHtSemiLayout sl;
	polr_htsemi_layout(shapes.data(), n_cols, plan.carried, kept, sl);
	const PolrHtFilterLayout &lo = sl.lo;
	DevBuf<uint8_t> col_mem;
	DevBuf<DevCol> keys_dev;
	HIPCHK(ctx, col_mem.alloc(lo.table_bytes));
	HIPCHK(ctx, keys_dev.alloc(ht->n_keys));
	std::vector<PolrHtFilterDesc> h_desc(sl.n_desc);
	std::vector<DevCol> h_keys(ht->n_keys);
	for (uint32_t c = 0; c < n_cols; c++) {
		const OwnedCol &col = hts_col(ht, c);
		PolrHtFilterDesc &d = h_desc[c];
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
	if (plan.carried) {
		// the row list the table has: one more 4-byte column, and its compacted copy is the composed list
		h_desc[n_cols] = PolrHtFilterDesc{(const uint8_t *)ht->filter_rows, nullptr, col_mem.get() + sl.list_off, nullptr, 4, 0};
	}
	PolrHtFilterDesc *desc = (PolrHtFilterDesc *)(col_mem.get() + lo.desc_off);
	uint32_t *rows = (uint32_t *)(col_mem.get() + lo.rows_off);
	HIPCHK(ctx, hipMemcpyAsync(keys_dev.get(), h_keys.data(), ht->n_keys * sizeof(DevCol), hipMemcpyHostToDevice, st));
	if (kept) {
		HIPCHK(ctx, hipMemcpyAsync(desc, h_desc.data(), sl.n_desc * sizeof(PolrHtFilterDesc), hipMemcpyHostToDevice, st));
		polr_launch_htfilter_compact(st, bits, tile_base, sc.n_tiles, desc, sl.n_desc, rows);
		HIPCHK(ctx, hipGetLastError());
	}
	HIPCHK(ctx, hipStreamSynchronize(st)); // (the table is complete; the staged arrays and the scratch are locals)
	// nothing can fail from here on: the table takes what was built and lets go of what it held
	uint64_t freed = ht->col_mem.bytes();
	for (uint32_t c = 0; c < n_cols; c++) {
		OwnedCol &col = hts_col(ht, c);
		freed += col.own_data.bytes() + col.own_valid.bytes();
		col.lib_cells = col.owned();
		col.own_data.reset();
		col.own_valid.reset();
		col.data = h_desc[c].dst_data;
		col.valid = h_desc[c].dst_valid;
	}
	ht->col_mem = std::move(col_mem); // (frees the allocation of a table filtered before or made by polr_ht_from_output)
	ht->keys_dev = std::move(keys_dev);
	ht->device_bytes = ht->device_bytes - freed + ht->col_mem.bytes();
	ht->n_rows_in = kept;
	ht->filter_rows = (uint32_t *)(ht->col_mem.get() + sl.list_off);
	ht->filtered = true;
	if (n_kept) {
		*n_kept = kept;
	}
	return POLR_OK;
}
