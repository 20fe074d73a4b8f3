// duckdb-polr_amd/csrc/polr_pool.hip -- the whole run in ONE launch (gfx950): routers + a pool of probe waves; the
// FLAT pipeline's kernel (the generic pipeline's: polr_poolg.hip).
//
// Grid: one WAVE per executor routes (the multiplexer of src/execution/operator/polr/physical_multiplexer.cpp:100-184
// with its RoutingStrategy, state in LDS for the whole run), every other wave is part of the probe pool.  A workgroup
// of this kernel owns its CU, so the routers sit INSIDE the probe workgroups, one or two in each (the mixed layout,
// pool_role): every CU issues probe requests.  Executor counts the workgroups' router areas cannot host take the
// separate layout -- the first `n_router_blocks` workgroups are routers only.  Protocol: polr_pool_device.h.  One
// kernel per compiled stage count K (-DPOLR_K):
//   polr_pool_flat_kernel<K>     the flat pipeline of polr_flat_device.h (counting runs over banks of single-key,
//                                unique-match joins on probe columns), up to 1024-thread workgroups that share the
//                                LDS-resident bit tables.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "polr_device.h"
#include "polr_mpx_device.h"

#ifndef POLR_K
#error "compile with -DPOLR_K=<compiled stage count>"
#endif

#ifndef POLR_FLAT_EMIT
#define POLR_FLAT_EMIT 0 // two builds per K: counting runs (0) and runs whose last join writes row ids (1)
#endif

#include "polr_pool_common.h"
#include "polr_flat_device.h"

static_assert(FLAT_STEP0 == POLR_POOL_GRAN_FLAT && FLAT_UNIT_MAX == POLR_POOL_UNIT_MAX, "the plan's unit sizes are the kernel's");

#define PASTE_TL2(a, b) a##b
#define PASTE_TL(a, b) PASTE_TL2(a, b)
#if !POLR_FLAT_EMIT
POOL_DIAG_ENTRY(PASTE_TL(polr_diag_router_k, POLR_K), PASTE_TL(polr_diag_timeline_set_k, POLR_K))
#endif

#if POLR_FLAT_EMIT
// every wave of the workgroup has left its loop (probe waves: EXIT; routers: finished): flush the cells of the fused
// sink that were touched to the workgroup's table.  Called by ALL waves of the workgroup.
__device__ __forceinline__ void flat_fused_flush(const DevOut &out, POLR_LDS unsigned long long *fused_lds, uint32_t fused_words) {
	__syncthreads();
	const FusedSink *f = out.fused;
	unsigned long long *table = f->cells + (size_t)(blockIdx.x % f->n_tables) * f->words_per_table;
	for (uint32_t i = threadIdx.x; i < fused_words; i += blockDim.x) {
		const unsigned long long v = fused_lds[i];
		if (v) {
			__hip_atomic_fetch_add(&table[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
	}
}
#endif

// (EMIT only tells the two builds' kernels apart by name: what differs is compiled in or out by POLR_FLAT_EMIT)
template <int K, int EMIT>
__global__ __launch_bounds__(1024) void polr_pool_flat_kernel(const DevPipeline *__restrict__ pipe,
                                                              const ResidentExec *__restrict__ execs, PoolRun *run,
                                                              DevOut out, uint32_t lds_per_wave, uint32_t table_dwords,
                                                              uint32_t router_dwords, uint32_t fused_off, uint32_t fused_words) {
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	const uint32_t wave_in_block = threadIdx.x >> 6;
	const uint32_t k = uni(pipe->k);
	PoolRun rh;
	pool_load_run(run, rh);
	const PoolRole role = pool_role(rh);
	const bool router_block = blockIdx.x < rh.n_router_blocks; // (the separate layout: nothing but routers here)
#if POLR_FLAT_EMIT
	// a fused GROUP BY sink whose cells fit: this workgroup's cells start from zero (published by the barrier below)
	if (router_block) {
		fused_words = 0;
	}
	POLR_LDS unsigned long long *fused_lds = fused_words ? as_lds((unsigned long long *)(lds + fused_off)) : nullptr;
	for (uint32_t i = threadIdx.x; i < fused_words; i += blockDim.x) {
		fused_lds[i] = 0ull;
	}
#endif
	// the bit tables that fit stay in LDS for the whole run: one cooperative copy per workgroup.  Router waves of a
	// probe workgroup take part in it and in its barrier.
	{
		const uint32_t n_tab = router_block ? 0u : uni(pipe->n_lds_tables);
		for (uint32_t t = 0; t < n_tab; t++) {
			const uint32_t *src = uniptr(pipe->lds_table_src[t]);
			const uint32_t off = uni(pipe->lds_table_off[t]);
			const uint32_t len = uni(pipe->lds_table_len[t]);
			for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) {
				lds[off + i] = src[i];
			}
		}
		__syncthreads();
	}
	if (role.router) {
		// a router of a probe workgroup: its area lies behind the probe queues of all waves; of a router workgroup:
		// wave r uses [r * router_dwords, (r + 1) * router_dwords)
		const uint32_t area = router_block ? router_dwords : POOL_ROUTER_MIN_DWORDS;
		uint32_t *base = lds + (router_block ? 0u : table_dwords + (blockDim.x >> 6) * lds_per_wave) + role.router_index * area;
		pool_router_wave(execs, run, rh, role.exec, k, FLAT_STEP0, base, area);
#if POLR_FLAT_EMIT
		if (fused_words) {
			flat_fused_flush(out, fused_lds, fused_words); // (with the probe waves: there is a barrier in it)
		}
#endif
		return;
	}
	// probe wave g of the pool serves ring g % n_rings (dealt wave by wave, not workgroup by workgroup: the units of a
	// round go to all rings alike, so every ring needs the same number of waves -- 240 workgroups over 64 rings left a
	// quarter of the rings with 3 workgroups instead of 4, and every round waited for those)
	const uint32_t pool_wave = role.pool_wave;
	const uint32_t ring = pool_wave & (rh.n_rings - 1u);
	FlatCtx<K> c;
	c.k = k;
	c.lane = threadIdx.x & 63;
	c.sel = as_global(uniptr(pipe->sel));
	c.plain = false; // (set with the first join order)
	c.lds_tables = as_lds((const uint32_t *)lds);
	c.q = as_lds((uint16_t *)(lds + table_dwords + (size_t)wave_in_block * lds_per_wave));
#pragma unroll
	for (int p = 0; p < K; p++) {
		c.qsize[p] = c.cnt[p] = 0;
		c.st[p].keys = nullptr;
		c.st[p].valid = nullptr;
		c.st[p].table = nullptr;
		c.st[p].kind_lds = c.st[p].a = c.st[p].b = c.st[p].out_slot = 0;
	}
	c.out = out;
	c.os = out_state_init();
#if POLR_FLAT_EMIT
	c.fused_lds = fused_lds;
#else
	c.fused_lds = nullptr;
#endif
	c.unit_begin = c.in_pos = c.in_end = 0;
	c.pf_pos = ~0ull;
	c.pf0 = make_uint4(0, 0, 0, 0);
	c.pf1 = make_uint4(0, 0, 0, 0);
	const FlatStageRec *flat_stages = uniptr(pipe->flat_stages);
	uint32_t cur_path = 0xFFFFFFFFu;
	PoolUnit u, nxt;
	PoolPoller pp;
	polr_pool_poller_init(pp, run, rh.sync, ring, rh.lo_cap, rh.hi_cap, pool_wave / rh.n_rings, rh.hi_lottery, rh.idle_sleep,
	                      rh.timeout_ticks);
	TL_BEGIN(pool_wave)
	bool have = polr_pool_next_unit(pp, u, c.lane);
	while (have) {
		TL_GOT
		const PoolArrival arrival = pool_arrival_of(execs, u, ring); // (asked for now, used when the unit is done)
		if (u.path != cur_path) {
			c.pf_pos = ~0ull; // (a prefetch belongs to one join order)
			flat_load_stages<K>(c.st, flat_stages, u.path);
			flat_set_plain<K>(c);
			cur_path = u.path;
		}
		TL_SWITCHED
#if POLR_FLAT_EMIT
		c.os.emit = u.emit != 0 && out.ids != nullptr && !c.os.overflow;
#endif
		c.unit_begin = u.begin;
		c.in_pos = u.begin;
		c.in_end = (uint64_t)u.begin + u.count;
		if (c.pf_pos != c.in_pos) {
			c.pf_pos = ~0ull;
		}
		flat_run_source<K>(c);
		TL_SOURCED
		// the source of this unit is used up: ONE look for the next unit before the queues drain, so that its claim and
		// the first keys of its source travel while this unit's last sweeps do (a unit's fixed cost is mostly dependent
		// round trips: measured 12.5 us + 6.3 ns per tuple)
		const uint32_t peek = polr_pool_look(pp, nxt);
		TL_LOOKED
		if (peek == POLR_POLL_WORK && nxt.path == cur_path) {
			flat_prefetch_unit<K>(c, nxt.begin, nxt.count);
		}
		flat_run_drain<K>(c);
		TL_RUN
		pool_arrive<K>(arrival, c.k, c.cnt);
		TL_DONE(u)
		if (peek == POLR_POLL_NONE) {
			have = polr_pool_next_unit(pp, nxt, c.lane);
		} else {
			have = peek == POLR_POLL_WORK;
		}
		u = nxt;
	}
#if POLR_FLAT_EMIT
	out_close(out, c.os, c.lane);
	if (fused_words) {
		flat_fused_flush(out, fused_lds, fused_words);
	}
#endif
}

// ---- launch ------------------------------------------------------------------------------------
#define PASTE2(a, b) a##b
#define PASTE(a, b) PASTE2(a, b)

static size_t pool_flat_wave_dwords() {
	return (size_t)flat_per_wave_dwords<POLR_K>();
}

// dynamic LDS of the flat kernel in dwords: tables + probe queues + the router areas of a probe workgroup (up to
// POOL_ROUTER_RESERVE, as many as fit: a function of the pipeline alone, not of the executors of a run), never less
// than a router workgroup's waves need (router wave r of a router workgroup uses [r * stride, (r + 1) * stride) with
// stride = total / waves).  How many routers a probe workgroup can host follows from it: polr_pool_flat_router_areas.
static size_t pool_flat_lds_dwords(uint32_t waves_per_block, uint32_t table_dwords) {
	const size_t probe = table_dwords + pool_flat_wave_dwords() * waves_per_block;
	const size_t room = probe < POOL_LDS_DWORDS_MAX ? (POOL_LDS_DWORDS_MAX - probe) / POOL_ROUTER_MIN_DWORDS : 0;
	const size_t mixed = probe + (size_t)POOL_ROUTER_MIN_DWORDS * (room < POOL_ROUTER_RESERVE ? room : POOL_ROUTER_RESERVE);
	const size_t router = (size_t)POOL_ROUTER_MIN_DWORDS * waves_per_block;
	return mixed > router ? mixed : router;
}

// the launch's LDS in bytes, a fused sink's cells (fused_words 8-byte words behind everything else) included
static size_t pool_flat_launch_lds(uint32_t waves_per_block, uint32_t table_dwords, uint32_t fused_words, uint32_t *fused_off) {
	const size_t dwords = pool_flat_lds_dwords(waves_per_block, table_dwords);
	const uint32_t off = (uint32_t)((dwords + 1) & ~(size_t)1);
	if (fused_off) {
		*fused_off = off;
	}
	return (fused_words ? (size_t)off + 2 * (size_t)fused_words : dwords) * sizeof(uint32_t);
}

static hipError_t pool_flat_prepare(size_t lds) {
	static size_t lds_set = 0;
	if (lds > lds_set) {
		hipError_t e = hipFuncSetAttribute((const void *)polr_pool_flat_kernel<POLR_K, POLR_FLAT_EMIT>,
		                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		if (e != hipSuccess) {
			return e;
		}
		lds_set = lds;
	}
	return hipSuccess;
}

#if POLR_FLAT_EMIT
#define FLAT_EXPORT(name) PASTE(PASTE(name, e_k), POLR_K)
#else
#define FLAT_EXPORT(name) PASTE(PASTE(name, k), POLR_K)
#endif

#if !POLR_FLAT_EMIT
// (LDS layout and waves per workgroup are the same in both builds; both keep 128 VGPRs)
extern "C++" size_t PASTE(polr_pool_flat_lds_bytes_k, POLR_K)(uint32_t waves_per_block, uint32_t table_dwords) {
	return pool_flat_lds_dwords(waves_per_block, table_dwords) * sizeof(uint32_t);
}

extern "C++" size_t PASTE(polr_pool_flat_wave_bytes_k, POLR_K)() {
	return pool_flat_wave_dwords() * sizeof(uint32_t);
}

// routers a probe workgroup can host (the mixed layout): the areas behind its probe queues
extern "C++" uint32_t PASTE(polr_pool_flat_router_areas_k, POLR_K)(uint32_t waves_per_block, uint32_t table_dwords) {
	const size_t probe = table_dwords + pool_flat_wave_dwords() * waves_per_block;
	const size_t areas = (pool_flat_lds_dwords(waves_per_block, table_dwords) - probe) / POOL_ROUTER_MIN_DWORDS;
	return (uint32_t)(areas < POOL_ROUTER_RESERVE ? areas : POOL_ROUTER_RESERVE);
}
#endif

// (fused_words: as for the launch -- the workgroups per CU of the launch as it will be made)
extern "C++" int FLAT_EXPORT(polr_pool_flat_occupancy_)(uint32_t waves_per_block, uint32_t table_dwords, uint32_t fused_words) {
	const size_t lds = pool_flat_launch_lds(waves_per_block, table_dwords, fused_words, nullptr);
	int blocks = 0;
	if (pool_flat_prepare(lds) != hipSuccess ||
	    hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, (const void *)polr_pool_flat_kernel<POLR_K, POLR_FLAT_EMIT>,
	                                                 (int)(64 * waves_per_block), lds) != hipSuccess) {
		return 0;
	}
	return blocks;
}

extern "C++" hipError_t FLAT_EXPORT(polr_launch_pool_flat_kernel_)(uint32_t n_blocks, uint32_t waves_per_block,
                                                                      uint32_t table_dwords, hipStream_t stream,
                                                                      const DevPipeline *pipe, const ResidentExec *execs,
                                                                      PoolRun *run, DevOut out, uint32_t fused_words) {
	// (fused_words: 64-bit group cells of a fused GROUP BY sink to keep in LDS behind everything else; 0: none)
	const size_t dwords = pool_flat_lds_dwords(waves_per_block, table_dwords);
	uint32_t fused_off = 0;
	const size_t lds = pool_flat_launch_lds(waves_per_block, table_dwords, fused_words, &fused_off);
	hipError_t e = pool_flat_prepare(lds);
	if (e != hipSuccess) {
		return e;
	}
	uint32_t per_wave = (uint32_t)pool_flat_wave_dwords();
	uint32_t router_dwords = (uint32_t)(dwords / waves_per_block);
	dim3 grid(n_blocks), block(64 * waves_per_block);
	uint32_t fused_off_arg = fused_words ? fused_off : 0u;
	void *args[] = {(void *)&pipe,         (void *)&execs,         (void *)&run,           (void *)&out,        (void *)&per_wave,
	                (void *)&table_dwords, (void *)&router_dwords, (void *)&fused_off_arg, (void *)&fused_words};
	return hipLaunchKernel((const void *)polr_pool_flat_kernel<POLR_K, POLR_FLAT_EMIT>, grid, block, args, lds, stream);
}
