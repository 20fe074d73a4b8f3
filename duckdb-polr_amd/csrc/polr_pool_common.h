// duckdb-polr_amd/csrc/polr_pool_common.h -- what the two pool kernels (flat pipeline: polr_pool.hip, generic pipeline:
// polr_poolg.hip) share on the device: loading the run header and an executor's descriptor into scalar registers, the
// router waves of a router workgroup, a probe wave's arrival, and the timeline records of the diagnostic build.
// The including file defines POOL_DIAG_SUFFIX (name suffix of the diagnostic entry points of ITS kernels).
#pragma once

#ifdef POLR_DIAG_TIMELINE
static __device__ unsigned long long polr_diag_router[16];
#endif
#include "polr_pool_device.h"

__device__ __forceinline__ void pool_load_run(const PoolRun *run, PoolRun &rh) {
	rh.sync = (PoolSync *)uni64((uint64_t)run->sync);
	rh.n_exec = uni(run->n_exec);
	rh.n_router_blocks = uni(run->n_router_blocks);
	rh.routers_per_block = uni(run->routers_per_block);
	rh.routers_rem = uni(run->routers_rem);
	rh.pool_waves = uni(run->pool_waves);
	rh.lo_cap = uni(run->lo_cap);
	rh.hi_cap = uni(run->hi_cap);
	rh.hi_tuples = uni(run->hi_tuples);
	rh.n_rings = uni(run->n_rings);
	rh.units_x = uni(run->units_x);
	rh.hi_unit = uni(run->hi_unit);
	rh.hi_lottery = uni(run->hi_lottery);
	rh.idle_sleep = uni(run->idle_sleep);
	rh.routers_done = 0;
	rh.abort = 0;
	rh.host_words = (volatile uint32_t *)uni64((uint64_t)run->host_words);
	rh.timeout_ticks = uni64(run->timeout_ticks);
	rh.share_recs = (uint32_t *)uni64((uint64_t)run->share_recs);
	rh.share_flags = (uint32_t *)uni64((uint64_t)run->share_flags);
	rh.share_stride = uni(run->share_stride);
	rh.share_after = uni(run->share_after);
}

__device__ __forceinline__ void pool_load_exec(const ResidentExec *xp, ResidentExec &x) {
	x.mpx = (DevMpx *)uni64((uint64_t)xp->mpx);
	x.sync = (ResidentSync *)uni64((uint64_t)xp->sync);
	x.counts = (unsigned long long *)uni64((uint64_t)xp->counts);
	x.chunk_begin = uni64(xp->chunk_begin);
	x.chunk_end = uni64(xp->chunk_end);
	x.chunk_offsets = (const uint64_t *)uni64((uint64_t)xp->chunk_offsets);
	x.n_chunks = uni64(xp->n_chunks);
	x.n_tuples = uni64(xp->n_tuples);
	x.flags = uni(xp->flags);
	x.pad = 0;
	x.stats_out = (polr_mpx_stats *)uni64((uint64_t)xp->stats_out);
	x.morsel_cursor = (unsigned long long *)uni64((uint64_t)xp->morsel_cursor);
	x.morsel_end = uni64(xp->morsel_end);
	x.morsel_chunks = uni(xp->morsel_chunks);
	x.path_plus1 = uni(xp->path_plus1);
	x.n_more = uni(xp->n_more);
	x.grant_chunks = uni(xp->grant_chunks);
	x.steal_words = (unsigned long long *)uni64((uint64_t)xp->steal_words);
#pragma unroll
	for (int j = 0; j < POLR_MORE_RANGES; j++) {
		x.more_begin[j] = uni64(xp->more_begin[j]);
		x.more_end[j] = uni64(xp->more_end[j]);
	}
}

// Who is who in the grid.  Separate layout: the first n_router_blocks workgroups are routers (wave w of workgroup b:
// executor b * waves + w), the others probe.  Mixed layout (n_router_blocks == 0): every workgroup probes, and its
// first waves route -- executor e in wave e / n_blocks of workgroup e % n_blocks.  Probe waves are numbered densely
// over the grid, router waves skipped: rings, the hi lottery and the EXIT count see pool_waves waves, no gaps.
struct PoolRole {
	bool router;
	uint32_t exec;          // router: its executor (>= n_exec: a spare wave of the last router workgroup)
	uint32_t router_index;  // router: which router of its workgroup
	uint32_t pool_wave;     // probe wave: its number in the pool
};
__device__ __forceinline__ PoolRole pool_role(const PoolRun &rh) {
	const uint32_t wave_in_block = threadIdx.x >> 6;
	const uint32_t wpb = blockDim.x >> 6;
	PoolRole r;
	if (blockIdx.x < rh.n_router_blocks) {
		r.router = true;
		r.exec = blockIdx.x * wpb + wave_in_block;
		r.router_index = wave_in_block;
		r.pool_wave = 0;
		return r;
	}
	const uint32_t pb = blockIdx.x - rh.n_router_blocks;
	const uint32_t mine = rh.routers_per_block + (pb < rh.routers_rem ? 1u : 0u);
	const uint32_t before = pb * rh.routers_per_block + (pb < rh.routers_rem ? pb : rh.routers_rem);
	r.router = wave_in_block < mine;
	r.exec = pb + wave_in_block * (gridDim.x - rh.n_router_blocks);
	r.router_index = wave_in_block;
	r.pool_wave = pb * wpb - before + wave_in_block - mine;
	return r;
}

// one router wave; base: its LDS area of router_dwords dwords
__device__ __forceinline__ void pool_router_wave(const ResidentExec *execs, PoolRun *run, const PoolRun &rh, uint32_t exec,
                                                 uint32_t k, uint32_t gran, uint32_t *base, uint32_t router_dwords) {
	if (exec >= rh.n_exec) {
		return;
	}
	// a router is one wave of mostly scalar-style, dependent code that everybody else waits for: it gets the SIMD's
	// issue slots ahead of the probe waves it shares the SIMD with
	__builtin_amdgcn_s_setprio(3);
	asm volatile("; polr-router-begin"); // (tools/spill_report.py tells the router's code from the probe loop's by these)
	ResidentExec x;
	pool_load_exec(execs + exec, x);
	const uint32_t cache_dwords = router_dwords - POOL_ROUTER_STATE - POOL_ROUTER_SAVE;
	polr_pool_router(x, run, rh, exec, k, gran, threadIdx.x & 63, base, (uint64_t *)(base + POOL_ROUTER_STATE + POOL_ROUTER_SAVE),
	                 cache_dwords / 2, base + POOL_ROUTER_STATE);
	asm volatile("; polr-router-end");
}

// diagnostic build only (-DPOLR_DIAG_TIMELINE, `make diag`; never compiled into the product): every probe wave writes
// {began waiting, got the unit, finished it, probing << 56 | exec << 40 | path << 32 | parts | count} per unit, 100 MHz wall
// clock; parts (flat kernel): three saturating 5-bit fields of quarter microseconds -- the join-order switch, the look for
// the next unit, the arrival -- so that probing - switch - look is the source and the drain (tools/diag_timeline.py)
#ifdef POLR_DIAG_TIMELINE
static __device__ unsigned long long *polr_diag_tl;
static __device__ uint32_t polr_diag_tl_cap;
#define TL_BEGIN(pool_wave_)                                                                                           \
	unsigned long long tl_wait = wall_clock64();                                                                       \
	unsigned long long tl_got = 0, tl_run = 0, tl_sw = 0, tl_src = 0, tl_look = 0;                                     \
	uint32_t tl_n = 0;                                                                                                 \
	const uint32_t tl_wave = (pool_wave_);
#define TL_GOT tl_got = wall_clock64();
#define TL_RUN tl_run = wall_clock64();
// (flat kernel) the unit's time in parts: .. join-order switch done .. source used up .. looked for the next unit
#define TL_SWITCHED tl_sw = wall_clock64();
#define TL_SOURCED tl_src = wall_clock64();
#define TL_LOOKED tl_look = wall_clock64();
/* a saturating 5-bit field of quarter microseconds (0 where the kernel does not take the two times) */
#define TL_Q5(from_, to_) ((from_) && (to_) > (from_) ? (((to_) - (from_)) / 25ull > 31ull ? 31ull : ((to_) - (from_)) / 25ull) : 0ull)
#define TL_DONE(u_)                                                                                                    \
	if (polr_diag_tl && tl_n < polr_diag_tl_cap && (threadIdx.x & 63) == 0) {                                          \
		unsigned long long *r_ = polr_diag_tl + ((size_t)tl_wave * polr_diag_tl_cap + tl_n) * 4;                       \
		r_[0] = tl_wait;                                                                                               \
		r_[1] = tl_got;                                                                                                \
		r_[2] = wall_clock64();                                                                                        \
		const unsigned long long q_ = (tl_run - tl_got) / 25ull; /* quarter microseconds spent probing, 8 bits */      \
		/* word 3: probing:8 | exec:16 | path:8 | arrival:5 | look:5 | switch:5 | count:17 (a unit is <= 65 536 tuples) */ \
		r_[3] = ((q_ > 255ull ? 255ull : q_) << 56) | ((unsigned long long)((u_).exec & 0xFFFFu) << 40) |              \
		        ((unsigned long long)(u_).path << 32) | (TL_Q5(tl_run, r_[2]) << 27) | (TL_Q5(tl_src, tl_look) << 22) | \
		        (TL_Q5(tl_got, tl_sw) << 17) | ((u_).count & 0x1FFFFu);                                               \
	}                                                                                                                  \
	tl_n++;                                                                                                            \
	tl_wait = wall_clock64();
// the host side of the diagnostic build: read (and reset) the routers' phase sums, install the timeline buffer
#define POOL_DIAG_ENTRY(router_name_, timeline_name_)                                                                  \
	extern "C" int router_name_(unsigned long long *dst, int reset) {                                                  \
		unsigned long long z[16] = {};                                                                                 \
		if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(polr_diag_router), sizeof(z)) != hipSuccess) {                         \
			return -1;                                                                                                 \
		}                                                                                                              \
		return reset ? (hipMemcpyToSymbol(HIP_SYMBOL(polr_diag_router), z, sizeof(z)) == hipSuccess ? 0 : -1) : 0;      \
	}                                                                                                                  \
	extern "C" int timeline_name_(unsigned long long *buf, uint32_t cap) {                                             \
		if (hipMemcpyToSymbol(HIP_SYMBOL(polr_diag_tl), &buf, sizeof(buf)) != hipSuccess) {                            \
			return -1;                                                                                                 \
		}                                                                                                              \
		return hipMemcpyToSymbol(HIP_SYMBOL(polr_diag_tl_cap), &cap, sizeof(cap)) == hipSuccess ? 0 : -1;              \
	}
#else
#define POOL_DIAG_ENTRY(router_name_, timeline_name_)
#define TL_BEGIN(pool_wave_)
#define TL_GOT
#define TL_RUN
#define TL_SWITCHED
#define TL_SOURCED
#define TL_LOOKED
#define TL_DONE(u_)
#endif

// Where a probe wave reports a unit: its counter bank [slot][ring & 7] and its arrival word.  Both hang on two pointers of
// the executor's descriptor, which are asked for when the unit is TAKEN (wave-uniform words of constant memory: scalar
// registers) -- they are home long before the unit ends, not one more round trip in front of its arrival.
struct PoolArrival {
	POLR_GLOBAL unsigned long long *bank;
	POLR_GLOBAL unsigned long long *arrived;
};
__device__ __forceinline__ PoolArrival pool_arrival_of(const ResidentExec *execs, const PoolUnit &u, uint32_t ring) {
	const POLR_CONST ResidentExec *xp = (const POLR_CONST ResidentExec *)uni64((uint64_t)execs) + uni(u.exec);
	const uint32_t shard = uni(ring) & (POLR_POOL_SHARDS - 1u), slot = uni(u.slot);
	PoolArrival a;
	a.bank = as_global(xp->counts) + (size_t)slot * POLR_NSHARD * POLR_KMAX + (size_t)shard * POLR_KMAX;
	a.arrived = as_global(&xp->sync->arrived[slot][shard].v);
	return a;
}

// a probe wave reports a finished unit: its stage counters, then the arrival -- ONE round trip for the counters: lane p
// adds counter p with one returning atomic instruction for all stages (a zero counter is left out by the lane mask), and
// the arrival consumes what came back, so it is issued after the adds have been performed.  (As first written lane 0
// issued up to K adds one after the other, each under its own branch and each waited for.)
template <int K>
__device__ __forceinline__ void pool_arrive(const PoolArrival &at, uint32_t k, uint32_t (&cnt)[K]) {
	const uint32_t lane = pool_lane_now(); // (asked for here: no lane mask of an arrival is worth a register pair across the unit)
	uint32_t mine = 0;
#pragma unroll
	for (int p = 0; p < K; p++) {
		mine = lane == (uint32_t)p ? cnt[p] : mine; // (the counters are wave-uniform: lane p gets counter p)
	}
	asm volatile("; polr-arrive-begin" ::: "memory");
	unsigned long long seen = 0;
	if (lane < k && mine) {
		seen = __hip_atomic_fetch_add(&at.bank[lane], (unsigned long long)mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	const unsigned long long late = __ballot((seen >> 63) != 0) != 0ull ? 1ull : 0ull;
	if (lane == 0) {
		__hip_atomic_fetch_add(at.arrived, POLR_POOL_TOKENS + late, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	asm volatile("; polr-arrive-end" ::: "memory");
#pragma unroll
	for (int p = 0; p < K; p++) {
		cnt[p] = 0;
	}
}

