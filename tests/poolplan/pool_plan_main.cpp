// tests/poolplan/pool_plan_main.cpp -- the pool launch plan (duckdb-polr_amd/csrc/polr_pool_plan.h) as a stand-alone host
// program: known answers, worked out from the formulas as they stood inside run_resident_impl before the plan became a
// function of its own, the invariants the device code relies on over a sweep of shapes, and how a round is cut into
// units (known answers and a fixed table of input -> unit lines).  Prints one line per check group, the table and "ok";
// any mismatch is printed and makes the exit status 1.
#include <stdio.h>
#include <string.h>

#include "../../duckdb-polr_amd/csrc/polr_pool_plan.h"

static int failures = 0;

#define CHECK(cond_, ...)                                                                                              \
	do {                                                                                                               \
		if (!(cond_)) {                                                                                                \
			printf("FAILED %s: ", #cond_);                                                                             \
			printf(__VA_ARGS__);                                                                                       \
			printf("\n");                                                                                              \
			failures++;                                                                                                \
		}                                                                                                              \
	} while (0)

struct Input {
	uint32_t n_cus;
	int occ;
	uint32_t share, flat, wpb, areas, n;
	uint64_t n_tuples;
};

struct Known {
	Input in;
	uint32_t mixed, n_router_blocks, n_blocks, pool_waves, n_rings, lo_cap, hi_cap, hi_lottery, hi_unit, routers_per_block,
	    routers_rem, ww0, ww_last;
};

// (wq only enters share_stride: 3 throughout)
static PoolPlan plan(const Input &in, const polr_pool_tuning &tn) {
	return polr_pool_plan(in.n_cus, in.occ, in.share, in.flat != 0, 3, in.wpb, in.areas, in.n, in.n_tuples, tn);
}

static const Known KNOWN[] = {
    {{256, 1, 1, 1, 16, 2, 1, 60000}, 1, 0, 256, 4095, 64, 4096, 256, 8, 1024, 0, 1, 64, 63},
    {{256, 1, 1, 1, 16, 2, 100, 60000}, 1, 0, 256, 3996, 64, 4096, 2048, 8, 1024, 0, 100, 63, 62},
    {{256, 1, 1, 1, 16, 2, 512, 60000}, 1, 0, 256, 3584, 64, 8192, 16384, 8, 1024, 2, 0, 56, 56},
    {{256, 1, 1, 1, 16, 2, 513, 60000}, 0, 33, 256, 3568, 64, 8192, 16384, 8, 1024, 0, 0, 56, 55},
    {{256, 1, 16, 1, 16, 2, 7, 60000}, 1, 0, 16, 249, 64, 512, 256, 2, 1024, 0, 7, 4, 3},
    {{256, 1, 16, 1, 16, 2, 20, 60000}, 1, 0, 16, 236, 64, 512, 512, 2, 1024, 1, 4, 4, 3},
    {{256, 1, 16, 1, 16, 2, 40, 60000}, 0, 3, 16, 208, 64, 1024, 1024, 2, 1024, 0, 0, 4, 3},
    {{256, 2, 1, 0, 4, 0, 8, 40000}, 0, 2, 512, 2040, 64, 2048, 256, 8, 64, 0, 0, 32, 31},
    {{256, 2, 1, 0, 4, 0, 100, 600000000ull}, 0, 25, 512, 1948, 64, 4096, 2048, 8, 256, 0, 0, 31, 30},
    {{256, 2, 16, 0, 4, 0, 1, 40000}, 0, 1, 32, 124, 64, 256, 128, 1, 64, 0, 0, 2, 1},
    {{256, 1, 16, 0, 4, 0, 60, 60000}, 0, 15, 16, 4, 4, 4096, 16384, 1, 64, 0, 0, 1, 1},
    {{256, 12, 1, 0, 4, 0, 8, 40000}, 0, 2, 2048, 8184, 64, 8192, 512, 8, 64, 0, 0, 128, 127}, // (occ clamps to 8)
    {{4, 1, 16, 1, 2, 2, 2, 1000}, 1, 0, 2, 2, 2, 512, 1024, 1, 1024, 1, 0, 1, 1},             // (areas clamp to wpb - 1)
};

static const Input NO_FIT[] = {
    {256, 1, 1, 1, 16, 0, 4096, 4000000000ull},
    {256, 1, 16, 1, 16, 2, 4096, 60000},
    {256, 1, 16, 0, 4, 0, 61, 60000},
    {4, 1, 16, 1, 2, 2, 3, 1000},
};

static void known_answers() {
	const polr_pool_tuning none = {};
	uint32_t rows = 0;
	for (const Known &k : KNOWN) {
		const PoolPlan p = plan(k.in, none);
#define ROW(field_, want_)                                                                                             \
	CHECK((uint32_t)(field_) == (want_), "row %u: %u, want %u", rows, (unsigned)(field_), (unsigned)(want_))
		CHECK(p.fits, "row %u", rows);
		ROW(p.mixed, k.mixed);
		ROW(p.n_router_blocks, k.n_router_blocks);
		ROW(p.n_blocks, k.n_blocks);
		ROW(p.pool_waves, k.pool_waves);
		ROW(p.n_rings, k.n_rings);
		ROW(p.lo_cap, k.lo_cap);
		ROW(p.hi_cap, k.hi_cap);
		ROW(p.hi_lottery, k.hi_lottery);
		ROW(p.hi_unit, k.hi_unit);
		ROW(p.routers_per_block, k.routers_per_block);
		ROW(p.routers_rem, k.routers_rem);
		ROW(p.worker_waves[0], k.ww0);
		ROW(p.worker_waves[p.n_rings - 1], k.ww_last);
		rows++;
	}
	uint32_t refused = 0;
	for (const Input &in : NO_FIT) {
		CHECK(!plan(in, none).fits, "no-fit input %u", refused);
		refused++;
	}
	printf("known answers: %u rows, %u refused\n", rows, refused);
}

static void tuning_answers() {
	const Input flat = KNOWN[0].in;
	Input generic = flat;
	generic.flat = 0;
	uint32_t checks = 0;
#define TUNED(in_, set_, field_, want_)                                                                                \
	do {                                                                                                               \
		polr_pool_tuning tn = {};                                                                                      \
		set_;                                                                                                          \
		const PoolPlan p = plan(in_, tn);                                                                              \
		CHECK(p.fits && (unsigned long long)p.field_ == (unsigned long long)(want_), "%s -> %s = %llu, want %llu", #set_,  \
		      #field_, (unsigned long long)p.field_, (unsigned long long)(want_));                                     \
		checks++;                                                                                                      \
	} while (0)
	TUNED(flat, tn.hi_lottery = 4, hi_lottery, 4);
	TUNED(flat, tn.hi_lottery = 16, hi_lottery, 8);
	TUNED(flat, tn.hi_unit = 128, hi_unit, 128);
	TUNED(flat, tn.units_x = 0, units_x, 4);
	TUNED(flat, tn.units_x = 2, units_x, 2);
	TUNED(flat, tn.hi_tuples_p1 = 0, hi_tuples, 4096);
	TUNED(flat, tn.hi_tuples_p1 = 1, hi_tuples, 0);
	TUNED(flat, tn.hi_tuples_p1 = 10000, hi_tuples, 4096);
	TUNED(flat, tn.idle_sleep = 16, idle_sleep, 16);
	TUNED(flat, tn.idle_sleep = 32, idle_sleep, 64);
	TUNED(flat, tn.idle_sleep = 0, idle_sleep, 64);
	TUNED(flat, tn.watchdog_us = 0, timeout_ticks, POLR_RES_TIMEOUT_TICKS);
	TUNED(flat, tn.watchdog_us = 5, timeout_ticks, 500);
	TUNED(flat, tn.share_after = 0, share_after, 0xFFFFFFFFu);
	TUNED(flat, tn.share_after = 16, share_after, 0xFFFFFFFFu);
	TUNED(flat, tn.share_after = 0xFFFFFFFFu, share_after, 0xFFFFFFFFu);
	TUNED(generic, tn.share_after = 0, share_after, 32);
	TUNED(generic, tn.share_after = 16, share_after, 16);
	for (uint32_t wq = 1; wq <= 9; wq++) {
		const polr_pool_tuning none = {};
		const PoolPlan p = polr_pool_plan(256, 1, 1, true, wq, 16, 2, 1, 60000, none);
		CHECK(p.share_stride == 8u + 64u * wq, "wq %u: share_stride %u", wq, p.share_stride);
		checks++;
	}
	printf("tuning answers: %u checks\n", checks);
}

static bool pow2(uint32_t v) {
	return v != 0 && (v & (v - 1)) == 0;
}

static void invariants() {
	static const uint32_t NS[] = {1, 2, 7, 63, 64, 65, 500, 4096}, WPBS[] = {2, 4, 8, 16}, CUS[] = {4, 256};
	const polr_pool_tuning none = {};
	uint32_t plans = 0, refused = 0;
	for (uint32_t n_cus : CUS)
	for (uint32_t flat = 0; flat < 2; flat++)
	for (uint32_t wpb : WPBS)
	for (uint32_t areas = 0; areas <= 3; areas++)
	for (int occ = 1; occ <= 8; occ++)
	for (uint32_t share = 1; share <= 16; share++)
	for (uint32_t n : NS) {
		const Input in = {n_cus, occ, share, flat, wpb, areas, n, 60000};
		const PoolPlan p = plan(in, none);
		const int before = failures;
		// (the refusal rule, worked out here from the inputs alone)
		const uint32_t capacity = n_cus * (uint32_t)occ / share > 2 ? n_cus * (uint32_t)occ / share : 2;
		const uint32_t hosts = areas < wpb - 1 ? areas : wpb - 1;
		const bool mixed = (uint64_t)n <= (uint64_t)capacity * hosts;
		const uint32_t n_router_blocks = mixed ? 0 : (n + wpb - 1) / wpb;
		CHECK(p.fits == !(n_router_blocks + 1 > capacity), "fits %d", (int)p.fits);
		if (!p.fits) {
			refused++;
		} else {
			plans++;
			CHECK(p.capacity == capacity && p.mixed == mixed && p.n_router_blocks == n_router_blocks, "layout");
			CHECK(pow2(p.n_rings) && p.n_rings <= 64 && p.n_rings <= p.pool_waves, "n_rings %u, pool_waves %u", p.n_rings,
			      p.pool_waves);
			uint64_t sum = 0;
			for (uint32_t r = 0; r < POLR_POOL_RINGS; r++) {
				CHECK(r < p.n_rings ? p.worker_waves[r] >= 1 : p.worker_waves[r] == 0, "worker_waves[%u] = %u", r,
				      p.worker_waves[r]);
				sum += p.worker_waves[r];
			}
			CHECK(sum == p.pool_waves, "worker waves sum to %llu of %u", (unsigned long long)sum, p.pool_waves);
			CHECK(pow2(p.lo_cap) && pow2(p.hi_cap), "lo_cap %u hi_cap %u", p.lo_cap, p.hi_cap);
			const uint32_t per_ring = p.pool_waves / p.n_rings;
			const uint32_t lot_max = per_ring < 1 ? 1 : (per_ring < 8 ? per_ring : 8);
			CHECK(pow2(p.hi_lottery) && p.hi_lottery <= lot_max, "hi_lottery %u, at most %u", p.hi_lottery, lot_max);
			if (p.mixed) {
				CHECK((uint64_t)p.routers_per_block * p.n_blocks + p.routers_rem == n, "routers %u x %u + %u", p.routers_per_block,
				      p.n_blocks, p.routers_rem);
				CHECK(p.pool_waves == p.n_blocks * wpb - n, "pool_waves %u", p.pool_waves);
				CHECK((uint64_t)n <= (uint64_t)p.capacity * hosts, "router areas");
			} else {
				CHECK(p.pool_waves == (p.n_blocks - p.n_router_blocks) * wpb, "pool_waves %u", p.pool_waves);
			}
		}
		if (failures != before) {
			printf("  at n_cus %u occ %d share %u flat %u wpb %u areas %u n %u\n", n_cus, occ, share, flat, wpb, areas, n);
		}
	}
	printf("invariants: %u plans, %u refused\n", plans, refused);
}

// how a round is cut into units (polr_pool_unit_size, the arithmetic of the routers' polr_pool_size_units), worked out
// by hand from the rule: <= hi_tuples: hi_unit; else ceil(tuples / max(16, units_x * pool_waves / active)) rounded up
// to gran, at most 65 536
struct UnitKnown {
	uint32_t tuples, pool_waves, active, gran, hi_tuples, units_x, hi_unit, unit, n_units;
};

static const UnitKnown UNIT_KNOWN[] = {
    // the 4096 boundary
    {4096, 4095, 1, 512, 4096, 4, 1024, 1024, 4},
    {4097, 4095, 1, 512, 4096, 4, 1024, 512, 9},
    {4097, 4095, 1, 64, 4096, 4, 64, 64, 65},
    {1000, 255, 1, 64, 4096, 4, 64, 64, 16},
    // ... moved by hi_tuples
    {1024, 255, 1, 512, 1024, 1, 320, 320, 4},
    {1025, 255, 1, 512, 1024, 1, 320, 512, 3},
    {0, 255, 1, 512, 0, 1, 1024, 1024, 0},
    {1, 255, 1, 512, 0, 1, 1024, 512, 1},
    // the floor of 16 on target: few probe waves, or many executors
    {100000, 8, 1, 64, 4096, 1, 64, 6272, 16},
    {100000, 255, 64, 512, 4096, 4, 1024, 6656, 16},
    // rounding up to gran 64 and gran 512
    {600000, 255, 1, 64, 4096, 1, 64, 2368, 254},
    {600000, 255, 1, 512, 4096, 1, 1024, 2560, 235},
    {652800, 255, 1, 512, 4096, 1, 1024, 2560, 255}, // (255 x 2560: the most tuples that still give units of 2560)
    {652801, 255, 1, 512, 4096, 1, 1024, 3072, 213},
    {652500, 255, 1, 64, 4096, 1, 64, 2560, 255},
    // the cap
    {16711680, 255, 1, 512, 4096, 1, 1024, 65536, 255}, // (255 x 65 536)
    {16781680, 255, 1, 512, 4096, 1, 1024, 65536, 257},
    {16781680, 255, 1, 64, 4096, 1, 64, 65536, 257},
    {4000000000u, 4095, 1, 512, 4096, 4, 1024, 65536, 61036},
    // several executors still routing (none: as one)
    {200000, 4095, 16, 512, 4096, 4, 1024, 512, 391},
    {200000, 2040, 8, 64, 4096, 4, 64, 256, 782},
    {200000, 255, 0, 512, 4096, 1, 1024, 1024, 196},
};

static void unit_answers() {
	uint32_t rows = 0;
	for (const UnitKnown &k : UNIT_KNOWN) {
		uint32_t unit = 0, n_units = 0;
		polr_pool_unit_size(k.tuples, k.pool_waves, k.active, k.gran, k.hi_tuples, k.units_x, k.hi_unit, &unit, &n_units);
		CHECK(unit == k.unit && n_units == k.n_units, "unit row %u: %u x %u, want %u x %u", rows, n_units, unit, k.n_units, k.unit);
		rows++;
	}
	printf("unit answers: %u rows\n", rows);
	// a fixed table, input -> unit: what tests/poolunits.py (the restatement the GPU tests size their sources with) is
	// held against, line by line
	static const uint32_t TUPLES[] = {0,      1,      4095,    4096,     4097,     20000,     130560,    200000,
	                                  652500, 652800, 652801,  1048576,  16711680, 16781680,  4294967295u};
	static const uint32_t WAVES[] = {2, 124, 255, 4095}, ACTIVE[] = {1, 3, 8}, GRAN[] = {64, 512}, UNITS_X[] = {1, 4};
	static const uint32_t HI[][2] = {{4096, 1024}, {4096, 64}, {1024, 320}, {0, 1024}}; // {hi_tuples, hi_unit}
	uint32_t lines = 0;
	for (uint32_t t : TUPLES)
	for (uint32_t w : WAVES)
	for (uint32_t a : ACTIVE)
	for (uint32_t g : GRAN)
	for (uint32_t x : UNITS_X)
	for (const uint32_t (&h)[2] : HI) {
		uint32_t unit = 0, n_units = 0;
		polr_pool_unit_size(t, w, a, g, h[0], x, h[1], &unit, &n_units);
		CHECK(unit >= 64 && unit <= POLR_POOL_UNIT_MAX && (uint64_t)unit * n_units >= t &&
		          (n_units == 0 || (uint64_t)unit * (n_units - 1) < t),
		      "units %u x %u do not cover %u tuples", n_units, unit, t);
		printf("unit %u %u %u %u %u %u %u -> %u %u\n", t, w, a, g, h[0], x, h[1], unit, n_units);
		lines++;
	}
	printf("unit table: %u lines\n", lines);
}

int main() {
	known_answers();
	tuning_answers();
	invariants();
	unit_answers();
	if (failures) {
		printf("%d check(s) failed\n", failures);
		return 1;
	}
	printf("ok\n");
	return 0;
}
