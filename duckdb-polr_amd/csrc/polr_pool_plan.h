// duckdb-polr_amd/csrc/polr_pool_plan.h -- the pool launch ("the whole run in one launch", polr_pool_device.h) as plain
// arithmetic: how many workgroups, where the routers sit, how many rings of what capacity, how rounds are cut into units.
// No HIP in here: the host side (polr_mpx.hip) calls polr_pool_plan() with what the occupancy functions told it, and a
// stand-alone host program checks it against known answers and its invariants (tests/poolplan/pool_plan_main.cpp).
// The constants the plan shares with the device code are defined here, once.
#pragma once

#include <stdint.h>

#include "../../include/polr_hip.h"

#define POLR_SLOTS 4 // rounds one executor can have in flight in a one-launch run (see ResidentSync)
#define POLR_RES_TIMEOUT_TICKS 400000000ull // 4 s of the 100 MHz wall clock: a wait this long is a lost run
#define POLR_POOL_RINGS 64 // unit queues; counters and arrivals are sharded 8 ways (ring & 7)
#define POLR_POOL_HI_TUPLES 4096u // rounds up to this many tuples are latency-critical (exploration slices)
#define POLR_POOL_HI_UNIT 64u // smallest unit of a small round (ring capacities are sized for it)

#define POLR_POOL_GRAN_FLAT 512u   // units of a big round are multiples of this many tuples: the flat kernel (a stage-0 step),
#define POLR_POOL_GRAN_GENERIC 64u // the generic kernel (one tuple per lane)
#define POLR_POOL_UNIT_MAX 65536u // most tuples per unit of a big round (the flat pipeline queues 16-bit unit positions)

// host and device: the qualifier is empty under a plain host compiler
#if defined(__HIPCC__) || defined(__CUDACC__)
#define POLR_PLAN_HD __host__ __device__ __forceinline__
#else
#define POLR_PLAN_HD static inline
#endif

// How a round of `tuples` tuples is cut into units (the routers: polr_pool_size_units, polr_pool_device.h).  A small
// round (<= hi_tuples) is cut into units of hi_unit tuples; a big one so that the executors still routing (`active`)
// each give every probe wave of their share of the pool about units_x units: ceil(tuples / target) tuples with
// target = max(16, units_x * pool_waves / active), rounded up to a multiple of `gran` (a power of two: 512 flat, 64
// generic), at most POLR_POOL_UNIT_MAX.
// (32-bit arithmetic: a round is at most 2^32 - 1 tuples, and the device has no integer divider -- a 64-bit division
// is a ~150-instruction sequence on the router's single lane)
// (Two expressions and their composition: the routers call the expressions from the branches in which they also pick
// the round's queue, which leaves their code as it was when the arithmetic stood there.)
POLR_PLAN_HD uint32_t polr_pool_big_unit(uint32_t tuples, uint32_t pool_waves, uint32_t active, uint32_t gran, uint32_t units_x) {
	uint32_t target = units_x * pool_waves / (active ? active : 1u);
	target = target < 16u ? 16u : target;
	uint32_t us = tuples / target + (tuples % target ? 1u : 0u);
	us = (us + gran - 1u) & ~(gran - 1u);
	return us < gran ? gran : (us > POLR_POOL_UNIT_MAX ? POLR_POOL_UNIT_MAX : us);
}
POLR_PLAN_HD uint32_t polr_pool_units_of(uint32_t tuples, uint32_t unit) {
	return tuples / unit + (tuples % unit ? 1u : 0u);
}
POLR_PLAN_HD void polr_pool_unit_size(uint32_t tuples, uint32_t pool_waves, uint32_t active, uint32_t gran, uint32_t hi_tuples,
                                      uint32_t units_x, uint32_t hi_unit, uint32_t *unit, uint32_t *n_units) {
	*unit = tuples <= hi_tuples ? hi_unit : polr_pool_big_unit(tuples, pool_waves, active, gran, units_x);
	*n_units = polr_pool_units_of(tuples, *unit);
}

static inline uint32_t next_pow2_u32(uint64_t v) {
	uint32_t p = 1;
	while (p < v) {
		p <<= 1;
	}
	return p;
}

struct PoolPlan {
	bool fits;                               // false: the executors do not fit on the device at once (nothing else is set)
	uint32_t capacity;                       // workgroups that are co-resident on this run's share of the device
	bool mixed;                              // the routers sit in the probe workgroups' first waves (else: router workgroups)
	uint32_t n_router_blocks, n_blocks;      // router workgroups in front of the grid (separate layout); the whole grid
	uint32_t routers_per_block, routers_rem; // mixed layout (PoolRun)
	uint32_t pool_waves;                     // all probe waves
	uint32_t n_rings;                        // rings in use
	uint32_t worker_waves[POLR_POOL_RINGS];  // probe waves that serve ring r
	uint32_t lo_cap, hi_cap;                 // entries per ring this run needs (powers of two)
	uint32_t units_x, hi_unit, hi_lottery, hi_tuples, idle_sleep; // as in PoolRun
	unsigned long long timeout_ticks;
	uint32_t share_after, share_stride;      // work sharing; share_after 0xFFFFFFFF: off
};

// n_cus: compute units of the device; occ: workgroups per CU, as the occupancy function returned it (>= 1); share: the
// run is sized for 1 / share of the device (resolved from the run's flags and the tuning); flat / wq / wpb /
// router_areas: the launch shape (flat pipeline? slots per queued tuple, waves per workgroup, routers a probe workgroup
// of the flat kernel can host in its LDS); n executors over a source of n_tuples; tn: polr_ctx_set_pool_tuning, 0 = default
static inline PoolPlan polr_pool_plan(uint32_t n_cus, int occ, uint32_t share, bool flat, uint32_t wq, uint32_t wpb,
                                      uint32_t router_areas, uint32_t n, uint64_t n_tuples, const polr_pool_tuning &tn) {
	PoolPlan pl = {};
	occ = occ < 8 ? occ : 8;
	// grid: never more than is co-resident.  Mixed layout (flat kernel, whose workgroup owns its CU): every workgroup
	// probes and hosts the routers of executors b, b + n_blocks, .. in its first waves -- as long as the router areas of
	// the workgroups (polr_pool_flat_router_areas, never all waves) can host all executors.  Else the separate layout:
	// router workgroups first (one wave per executor), then the pool.  (The generic kernel runs two workgroups per CU
	// with its LDS nearly used up: router areas there would cost the second workgroup; it keeps router workgroups.)
	const uint32_t co_resident = n_cus * (uint32_t)occ / share;
	pl.capacity = co_resident > 2u ? co_resident : 2u;
	router_areas = router_areas < wpb - 1u ? router_areas : wpb - 1u;
	pl.mixed = (uint64_t)n <= (uint64_t)pl.capacity * router_areas;
	pl.n_router_blocks = pl.mixed ? 0u : (n + wpb - 1) / wpb;
	if (pl.n_router_blocks + 1 > pl.capacity) {
		return pl;
	}
	pl.fits = true;
	pl.n_blocks = pl.capacity;
	pl.routers_per_block = pl.mixed ? n / pl.n_blocks : 0u;
	pl.routers_rem = pl.mixed ? n % pl.n_blocks : 0u;
	// unit rings: sized for everything the executors of this run can have in flight (two slots each) plus the EXIT
	// entries, with a factor of two to spare
	const uint32_t pool_waves = pl.mixed ? pl.n_blocks * wpb - n : (pl.n_blocks - pl.n_router_blocks) * wpb;
	pl.pool_waves = pool_waves;
	// Rings in use: every ring must have probe waves that serve it.  Ring capacity: a round of U units leaves at most
	// U / R + 1 entries on a ring; the executors that have rounds in flight (a of them, at most POLR_SLOTS rounds each) published them
	// when at least a executors were still routing, so all their lo units together are at most POLR_SLOTS x (4 x pool_waves + 17 a);
	// a hi round has at most POLR_POOL_HI_TUPLES / 64 units.  Twice that, plus the EXIT entries.
	uint32_t n_rings = 1;
	while (n_rings * 2 <= (pool_waves < POLR_POOL_RINGS ? pool_waves : (uint32_t)POLR_POOL_RINGS)) {
		n_rings *= 2;
	}
	pl.n_rings = n_rings;
	const uint64_t R = n_rings;
	// (+ a round larger than target x 65 536 tuples has tuples / 65 536 units)
	pl.lo_cap = next_pow2_u32(2ull * ((4ull * POLR_SLOTS * pool_waves + 17ull * POLR_SLOTS * n +
	                                   (uint64_t)POLR_SLOTS * (n_tuples >> 16)) / R +
	                                  (uint64_t)POLR_SLOTS * n + pool_waves / R + 16) + 64);
	// (+ work sharing: a probe wave has at most one shared piece outstanding, published on the ring after its own)
	pl.hi_cap = next_pow2_u32(
	    2ull * ((uint64_t)POLR_SLOTS * n * (POLR_POOL_HI_TUPLES / POLR_POOL_HI_UNIT / R + 1) + pool_waves / R + 1) + 64);
	for (uint32_t r = 0; r < POLR_POOL_RINGS; r++) {
		pl.worker_waves[r] = r < n_rings ? (pool_waves + n_rings - 1 - r) / n_rings : 0u; // (wave g serves ring g % n_rings)
	}
	pl.units_x = tn.units_x ? tn.units_x : 4u; // (ring capacities are sized for 4)
	{
		// the fewest probe waves any ring has; the lottery divides them into at most 8 classes
		const uint32_t min_waves = pool_waves / n_rings;
		uint32_t lot = 1;
		while (lot * 2 <= (min_waves < 8u ? min_waves : 8u)) {
			lot *= 2;
		}
		pl.hi_lottery = (tn.hi_lottery >= 1 && tn.hi_lottery <= lot) ? tn.hi_lottery : lot;
	}
	// tuples per unit of a small round.  Default: flat: two steps of the pipeline's stage 0 (1 024 tuples = one
	// exploration slice of init_tuple_count in one
	// unit: measured 1.52 ms against 1.55-1.56 with 512 on the SF100 run), generic: a wide step of 256.  64-tuple units
	// finish a lone small round soonest, but a unit costs its wave the same chain of dependent round trips whatever
	// its size, and with hundreds of executors exploring that wave time is what the pool runs out of (measured on
	// the SF100 run: 2.29 ms with 64-tuple units, 1.77 ms with 512)
	// (generic pipelines with few executors: 64 -- an exploration slice spread over 16 waves; measured on the 113
	// JOB-shaped pipelines, 8 executors each: 46.9 ms per pass against 47.4 with 128 and 49.8 with 256)
	pl.hi_unit = tn.hi_unit ? tn.hi_unit : (flat ? 1024u : (n <= 64u ? 64u : 256u));
	// (the size up to which a round is latency-critical)
	pl.hi_tuples = tn.hi_tuples_p1 ? (tn.hi_tuples_p1 - 1u < POLR_POOL_HI_TUPLES ? tn.hi_tuples_p1 - 1u : POLR_POOL_HI_TUPLES)
	                               : POLR_POOL_HI_TUPLES;
	pl.idle_sleep = tn.idle_sleep == 16 ? 16u : 64u; // (an idle probe wave's longest back-off)
	// watchdog: ticks of the 100 MHz wall clock (default 4 s: a wait this long is a lost run)
	pl.timeout_ticks = tn.watchdog_us ? (unsigned long long)tn.watchdog_us * 100ull : POLR_RES_TIMEOUT_TICKS;
	// work sharing (generic pipeline only): records of 8 + 64 x (words per queued tuple) dwords, one per probe wave, and
	// their flags -- all flags are 0 between runs (a record is released by the wave that took it) unless a run was given up
	pl.share_after = flat ? 0xFFFFFFFFu : (tn.share_after ? tn.share_after : 32u);
	pl.share_stride = 8u + 64u * wq;
	return pl;
}
