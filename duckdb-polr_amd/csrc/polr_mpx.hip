// duckdb-polr_amd/csrc/polr_mpx.hip -- device-resident multiplexer.
//
// The reference asks its multiplexer for a route once per 1024-tuple chunk on the host
// (POLARPipelineExecutor::Execute, src/parallel/polar_pipeline_executor.cpp:320-366).  Here the
// multiplexer state (PhysicalMultiplexer + RoutingStrategy, polr_routing.h) lives on the device and one
// *routing step* (polr_mpx_device.h) runs between two probe rounds:
//
//     absorb the k counters of the previous round (AddNumIntermediates), FinalizePathRun, Route the next slice,
//     fold the strategy's routing window (num_cache_flushing_skips whole chunks that bypass routing, :322-329)
//     into the same round, publish the round
//
// Two ways to drive it, same decisions, same results (this file is their host side):
//   * polr_mpx_run / _run_many: one launch of the path kernel per round; its last busy workgroup runs the step
//     for the next round; the host pumps launches, throttled by two pinned progress words;
//   * polr_mpx_run_resident: the whole run is one launch; per executor a router wave keeps the state in LDS
//     and probe workgroups wait for its rounds on the device.
// Output row sets and per-round intermediates equal the host classes' exactly: same code (polr_routing.h), same
// IEEE double arithmetic.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "polr_internal.h"
#include "polr_mpx_device.h"
#include "polr_pool_device.h"

struct polr_mpx {
	polr_pipeline *pipe = nullptr;
	polr_ctx *ctx = nullptr; // (kept so that destroying the object never has to go through the pipeline)
	polr_mpx_config cfg;
	DevBuf<DevMpx> dev;
	DevBuf<DevRound> round_dev;
	DevBuf<uint64_t> prefix_dev;
	DevBuf<uint32_t> unit_size_dev;
	DevBuf<uint32_t> ticket_dev;
	DevBuf<polr_mpx_stats> stats_dev;
	DevBuf<unsigned long long> stamps_dev; // diagnostic builds only
	uint32_t iter = 0; // launches of the path kernel so far (descriptor slot = iter & 1)
	DevBuf<unsigned long long> counts_dev;
	// the chunk boundaries in use: a view of chunk_offsets_own (polr_mpx_set_chunk_offsets), or of the pipeline's scan
	// result (polr_mpx_use_scan_chunks: from_scan, of the scan scan_generation); nullptr: chunks of cfg.chunk_size tuples
	uint64_t *chunk_offsets_dev = nullptr;
	DevBuf<uint64_t> chunk_offsets_own;
	bool from_scan = false;
	uint64_t scan_generation = 0;
	DevBuf<uint32_t> log_path;
	DevBuf<uint64_t> log_tuples, log_inter;
	volatile uint32_t *done_host = nullptr;    // pinned, mapped: the words the device reports in (PolrHostWord)
	volatile uint32_t *progress_dev = nullptr; // the device's view of done_host
	uint32_t steps_base = 0;
	bool pending_sync = false;
	hipStream_t own_stream = nullptr;  // used when the caller passes no stream
	hipStream_t last_stream = nullptr; // where the queued tail of the last run sits
	uint32_t unit_size = 256;
	uint32_t wide0_mask = 0;
	uint64_t n_chunks = 0;
	// resident launches
	DevBuf<ResidentSync> sync_dev;     // arrival counters of this executor
	DevBuf<char> execs_dev;            // run header + executor descriptors + morsel cursor (owned by the first multiplexer of a run)
	uint32_t execs_cap = 0;            // executor descriptors execs_dev is laid out for
	std::vector<char> execs_host;      // what execs_dev holds (a pass that repeats the last one re-sends nothing)
	DevBuf<uint8_t> pool_dev;          // unit rings of the runs this multiplexer leads: a PoolSync and the rings behind it
	DevBuf<uint32_t> share_dev;        // work sharing of the generic pipeline: one record per probe wave + its flag
	uint32_t pool_lo_cap = 0, pool_hi_cap = 0; // ring capacities pool_dev is laid out for
	bool pool_dirty = false;           // a run was given up: rings and tickets are re-initialised before the next one
	polr_mpx *leader = nullptr;        // the first multiplexer of the last pool run this one took part in (owns the rings)
	uint32_t res_epoch = 0;
	polr_mpx_stats *stats_host = nullptr; // pinned, mapped: closing statistics of a POLR_RUN_FINISH run
	polr_mpx_stats *stats_host_dev = nullptr;
	bool stats_in_host = false;
	// range stealing (polr_mpx_run_resident_stealing): the claim words of the runs this multiplexer leads + the
	// executors' counters behind them, and what they are initialised from with every launch
	DevBuf<unsigned long long> steal_dev; // [5 per executor]
	std::vector<unsigned long long> steal_host;
	bool steal_run = false;            // the last run of this multiplexer was a stealing run (its counters are in done_host)
	polr_steal_stats steal_stats = {}; // picked up by polr_mpx_finish(_many)
	// optional per-launch timing (measurement only)
	bool timing = false;
	std::vector<hipEvent_t> ev_start, ev_stop;
	size_t ev_used = 0;
	double timed_ms = 0;
	uint64_t timed_launches = 0;
};

// every multiplexer keeps its work on ONE stream at a time: the caller's, else the stream of its last run
// (a resident run puts all its executors on one stream), else its own
static hipStream_t pick_stream(polr_mpx *m, void *stream) {
	return stream ? (hipStream_t)stream : (m->last_stream ? m->last_stream : m->own_stream);
}

// move a multiplexer onto `st`: whatever it still has queued elsewhere must be finished first
static hipError_t adopt_stream(polr_mpx *m, hipStream_t st) {
	const hipStream_t prev = m->last_stream ? m->last_stream : m->own_stream;
	hipError_t e = hipSuccess;
	if (prev != st) {
		e = hipStreamSynchronize(prev);
		m->pending_sync = false;
	}
	m->last_stream = st;
	return e;
}

// after the stream of a run has been synchronised: the stealing counters its router left in the pinned words
static void collect_steal_stats(polr_mpx *m) {
	memset(&m->steal_stats, 0, sizeof(m->steal_stats));
	if (m->steal_run) {
		m->steal_stats.chunks_routed = m->done_host[POLR_HW_CHUNKS_ROUTED];
		m->steal_stats.chunks_stolen = m->done_host[POLR_HW_CHUNKS_STOLEN];
		m->steal_stats.n_steals = m->done_host[POLR_HW_STEALS];
	}
}

// optional per-launch timing: take the next event pair of `m` (made on demand) and record its start on `st` ...
static int timing_start(polr_mpx *m, hipStream_t st, size_t *ev) {
	if (!m->timing) {
		return POLR_OK;
	}
	polr_ctx *ctx = m->pipe->ctx;
	*ev = m->ev_used++;
	if (*ev >= m->ev_start.size()) {
		hipEvent_t a, b;
		HIPCHK(ctx, hipEventCreate(&a));
		HIPCHK(ctx, hipEventCreate(&b));
		m->ev_start.push_back(a);
		m->ev_stop.push_back(b);
	}
	HIPCHK(ctx, hipEventRecord(m->ev_start[*ev], st));
	return POLR_OK;
}

// ... and its stop, behind the launch
static int timing_stop(polr_mpx *m, hipStream_t st, size_t ev) {
	if (m->timing) {
		HIPCHK(m->pipe->ctx, hipEventRecord(m->ev_stop[ev], st));
	}
	return POLR_OK;
}

static void drain_events(polr_mpx *m) {
	for (size_t i = 0; i < m->ev_used; i++) {
		float ms = 0;
		if (hipEventElapsedTime(&ms, m->ev_start[i], m->ev_stop[i]) == hipSuccess) {
			m->timed_ms += ms;
			m->timed_launches++;
		}
	}
	m->ev_used = 0;
}

__global__ void polr_mpx_init_kernel(DevMpx *m, polr_mpx_config cfg, uint32_t n_paths, uint64_t n_tuples,
                                     uint64_t n_chunks, uint32_t *log_path, uint64_t *log_tuples,
                                     uint64_t *log_inter, uint32_t wide0_mask, volatile uint32_t *progress,
                                     uint32_t steps_done_init) {
	m->wide0_mask = wide0_mask;
	m->cfg = cfg;
	m->n_paths = n_paths;
	m->pad2 = 0;
	m->progress = progress;
	m->steps_done = steps_done_init; // monotonic across resets: the host throttles on differences
	m->pad3 = 0;
	m->core.Init(cfg.routing, n_paths, cfg.regret_budget, cfg.init_tuple_count, cfg.atc_multiplier);
	m->chunk_idx = m->chunk_end = 0;
	m->n_tuples = n_tuples;
	m->n_chunks = n_chunks;
	m->chunk_size = cfg.chunk_size;
	m->done = 1;
	m->chunk_offsets = nullptr;
	m->num_intermediates_total = 0;
	m->num_rounds = 0;
	m->log_enabled = cfg.log_rounds;
	m->max_log = cfg.max_log_rounds;
	m->n_log = 0;
	m->log_path = log_path;
	m->log_tuples = log_tuples;
	m->log_inter = log_inter;
	m->last_path = 0;
	for (uint32_t p = 0; p < POLR_MAX_PATHS; p++) {
		for (uint32_t j = 0; j < POLR_MAX_JOINS; j++) {
			m->stage_out[p][j] = 0;
		}
	}
	// (one thread: runs once per pass, ~300 stores)
}

__global__ void polr_mpx_set_range_kernel(DevMpx *m, uint64_t chunk_begin, uint64_t chunk_end,
                                          const uint64_t *chunk_offsets, uint64_t n_chunks, uint64_t n_tuples) {
	m->chunk_idx = chunk_begin;
	m->chunk_end = chunk_end;
	m->chunk_offsets = chunk_offsets;
	m->n_chunks = n_chunks;
	m->n_tuples = n_tuples;
	m->done = chunk_begin >= chunk_end ? 1 : 0;
}

// stand-alone routing step: primes the first round of a run (later rounds are routed by the last
// workgroup of each path-kernel launch)
__global__ void polr_mpx_router_kernel(DevMpx *m, DevRound *round, uint64_t *unit_prefix, uint32_t *unit_size_out,
                                       unsigned long long *counts, uint32_t k, uint32_t resident_waves) {
	polr_router_step(m, round, unit_prefix, unit_size_out, counts, k, resident_waves, threadIdx.x, false, nullptr);
}

// PushFinalize's closing FinalizePathRun (polar_pipeline_executor.cpp:150-151); one wave
__global__ void polr_mpx_finish_kernel(DevMpx *m, unsigned long long *counts, uint32_t k, polr_mpx_stats *stats) {
	const uint32_t lane = threadIdx.x;
	polr::MultiplexerCore &core = m->core;
	uint64_t s = 0;
	for (uint32_t j = 0; j < k; j++) {
		unsigned long long v = 0;
		if (lane < POLR_NSHARD) {
			v = counts[(uint64_t)lane * k + j];
			counts[(uint64_t)lane * k + j] = 0;
		}
		for (int d = 32; d > 0; d >>= 1) {
			v += __shfl_down(v, d, 64);
		}
		if (lane == 0) {
			s += v;
			m->stage_out[m->last_path][j] += v;
		}
	}
	if (lane == 0) {
		core.AddNumIntermediates(s);
		m->num_intermediates_total += s;
		polr_close_run(m);
	}
	__syncthreads();
	polr_write_stats(m, m, stats, lane);
}

extern "C" {

int polr_mpx_create(polr_pipeline *p, const polr_mpx_config *cfg, polr_mpx **out) {
	POLR_ENTRY();
	if (!p || !cfg || !out) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = p->ctx;
	*out = nullptr;
	if (cfg->routing > POLR_ROUTE_EXPONENTIAL_BACKOFF) {
		POLR_FAIL(ctx, POLR_E_INVALID, "unknown routing strategy %u", cfg->routing);
	}
	if (cfg->chunk_size < 2 || cfg->chunk_size > 65536) {
		POLR_FAIL(ctx, POLR_E_INVALID, "chunk size %u out of range", cfg->chunk_size);
	}
	if (p->n_paths > polr::kMaxPaths) {
		POLR_FAIL(ctx, POLR_E_UNSUPPORTED, "too many join orders");
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	polr_mpx *m = new polr_mpx();
	m->pipe = p;
	m->ctx = polr_ctx_retain(p->ctx);
	m->cfg = *cfg;
	m->n_chunks = (p->n_tuples + cfg->chunk_size - 1) / cfg->chunk_size;
	const uint64_t max_log = cfg->log_rounds ? std::max<uint64_t>(cfg->max_log_rounds, 1) : 1;
	hipError_t e = m->dev.alloc(1);
	e = e == hipSuccess ? m->round_dev.alloc(2) : e;
	e = e == hipSuccess ? m->prefix_dev.alloc(4) : e;
	e = e == hipSuccess ? m->unit_size_dev.alloc(2) : e;
	e = e == hipSuccess ? m->ticket_dev.alloc(16) : e;
	e = e == hipSuccess ? hipStreamCreateWithFlags(&m->own_stream, hipStreamNonBlocking) : e;
	e = e == hipSuccess ? hipMemset(m->ticket_dev, 0, 64) : e;
	// two counter banks (a resident run keeps up to two rounds in flight; everything else uses the first)
	e = e == hipSuccess ? m->counts_dev.alloc(POLR_SLOTS * POLR_NSHARD * POLR_KMAX) : e;
	e = e == hipSuccess ? m->log_path.alloc(max_log) : e;
	e = e == hipSuccess ? m->log_tuples.alloc(max_log) : e;
	e = e == hipSuccess ? m->log_inter.alloc(max_log) : e;
	e = e == hipSuccess ? hipHostMalloc((void **)&m->done_host, POLR_HOST_WORDS_BYTES, hipHostMallocMapped) : e;
	if (e == hipSuccess) {
		memset((void *)m->done_host, 0, POLR_HOST_WORDS_BYTES);
		e = hipHostGetDevicePointer((void **)&m->progress_dev, (void *)m->done_host, 0);
	}
	e = e == hipSuccess ? hipMemset(m->counts_dev, 0, POLR_SLOTS * POLR_NSHARD * POLR_KMAX * 8) : e;
	e = e == hipSuccess ? m->sync_dev.alloc(1) : e;
	e = e == hipSuccess ? hipHostMalloc((void **)&m->stats_host, sizeof(polr_mpx_stats), hipHostMallocMapped) : e;
	e = e == hipSuccess ? hipHostGetDevicePointer((void **)&m->stats_host_dev, m->stats_host, 0) : e;
	e = e == hipSuccess ? hipMemset(m->sync_dev, 0, sizeof(ResidentSync)) : e;
	if (e != hipSuccess) {
		polr_mpx_destroy(m);
		POLR_FAIL(ctx, POLR_E_HIP, "multiplexer allocation failed: %s", hipGetErrorString(e));
	}
	m->cfg.max_log_rounds = (uint32_t)max_log;
	// every stage 0 takes wide (256-tuple) steps, so units are multiples of 256 tuples
	m->wide0_mask = p->n_paths >= 32 ? 0xFFFFFFFFu : ((1u << p->n_paths) - 1u);
	// (zero first: the bookkeeping of resident runs, res_valid / res_target, is not touched by the init kernel --
	// a host-side reset keeps it)
	e = hipMemsetAsync(m->dev, 0, sizeof(DevMpx), ctx->stream);
	if (e != hipSuccess) {
		polr_mpx_destroy(m);
		POLR_FAIL(ctx, POLR_E_HIP, "multiplexer init failed: %s", hipGetErrorString(e));
	}
	hipLaunchKernelGGL(polr_mpx_init_kernel, dim3(1), dim3(1), 0, ctx->stream, m->dev, m->cfg, p->n_paths, p->n_tuples,
	                   m->n_chunks, m->log_path, m->log_tuples, m->log_inter, m->wide0_mask, m->progress_dev, 0u);
	e = hipStreamSynchronize(ctx->stream);
	if (e != hipSuccess) {
		polr_mpx_destroy(m);
		POLR_FAIL(ctx, POLR_E_HIP, "multiplexer init failed: %s", hipGetErrorString(e));
	}
	*out = m;
	return POLR_OK;
}

int polr_mpx_set_chunk_offsets(polr_mpx *m, const uint64_t *offsets, uint64_t n_chunks) {
	POLR_ENTRY();
	if (!m || (!offsets && n_chunks)) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = m->pipe->ctx;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	m->chunk_offsets_own.reset();
	m->chunk_offsets_dev = nullptr;
	m->from_scan = false;
	if (!offsets) {
		m->n_chunks = (m->pipe->n_tuples + m->cfg.chunk_size - 1) / m->cfg.chunk_size;
		return POLR_OK;
	}
	for (uint64_t c = 0; c < n_chunks; c++) {
		if (offsets[c + 1] < offsets[c] || offsets[c + 1] > m->pipe->n_tuples) {
			POLR_FAIL(ctx, POLR_E_INVALID, "chunk offsets must be non-decreasing and within the %llu source tuples",
			          (unsigned long long)m->pipe->n_tuples);
		}
	}
	HIPCHK(ctx, m->chunk_offsets_own.alloc(n_chunks + 1));
	m->chunk_offsets_dev = m->chunk_offsets_own;
	HIPCHK(ctx, hipMemcpy(m->chunk_offsets_dev, offsets, (n_chunks + 1) * 8, hipMemcpyHostToDevice));
	m->n_chunks = n_chunks;
	return POLR_OK;
}

// A pool launch about to be enqueued on `st`, sized for 1 / share of the device: make `st` wait for the pool launches of
// OTHER streams it cannot run beside -- all of them if this one takes the whole device, the full-size ones otherwise
// (launches that each declared a share, POLR_RUN_SHARE, are the caller's to add up) -- and open the entry whose event the
// caller records behind the launch.  Same-stream launches are ordered by the stream.
static int order_pool_launch(polr_ctx *ctx, hipStream_t st, uint32_t share) {
	// (the lists change only when every call below has succeeded)
	std::vector<polr_ctx::PoolLaunch> keep;
	std::vector<hipEvent_t> retired;
	for (auto &f : ctx->pool_launches) {
		bool retire = f.stream == st; // (superseded: this stream's next launch carries the newer event)
		if (!retire && (share <= 1 || f.share <= 1)) {
			HIPCHK(ctx, hipStreamWaitEvent(st, f.done, 0));
			retire = share <= 1; // (everything enqueued later waits for THIS launch, which waits for f)
		}
		if (retire) {
			retired.push_back(f.done);
		} else {
			keep.push_back(f);
		}
	}
	hipEvent_t done = nullptr;
	if (!retired.empty()) {
		done = retired.back();
		retired.pop_back();
	} else if (!ctx->pool_events_free.empty()) {
		done = ctx->pool_events_free.back();
		ctx->pool_events_free.pop_back();
	} else {
		HIPCHK(ctx, hipEventCreateWithFlags(&done, hipEventDisableTiming));
	}
	ctx->pool_events_free.insert(ctx->pool_events_free.end(), retired.begin(), retired.end());
	keep.push_back({st, done, share});
	ctx->pool_launches.swap(keep);
	return POLR_OK;
}

// The shape of a pool launch of pipeline `p`: which kernel, on which descriptors, how wide its workgroups are and how
// many of them a CU holds.  (The part of the preparation that asks the kernels' own occupancy and LDS functions.)
struct PoolShape {
	bool flat;             // the flat pipeline's kernel (polr_pool.hip), else the generic one (polr_poolg.hip)
	const DevPipeline *dp; // the variant of the pipeline's descriptors the launch runs on
	uint32_t wq;           // slots per queued tuple: ids (+ multiplicity)
	uint32_t wpb;          // waves per workgroup; 0: does not fit at all
	uint32_t fused_words;  // 8-byte cells of a fused GROUP BY sink the launch keeps in LDS
	uint32_t router_areas; // routers a probe workgroup of the flat kernel can host in its own LDS
	int occ;               // workgroups per CU, as the occupancy function returned it; < 1: does not fit on a CU
};

static PoolShape pool_shape(polr_pipeline *p, bool materialize, const polr_out *out) {
	PoolShape sh;
	// a bank of single-key unique-match joins takes the flat pipeline -- counting runs always, emitting runs when every
	// join is a perfect table (polr_flat_device.h); it runs on the counting variant's descriptors either way
	// (an output with a fused UNGROUPED sink is filled by the generic kernel alone -- gen_out_write is where its tuples
	// are folded --, over the materialising descriptors, whatever the pipeline's emitting runs would otherwise take)
	const bool agg_sink = materialize && out && out->agg_dev;
	sh.flat = p->host_count.flat != 0 && (!materialize || p->flat_emit) && !agg_sink;
	const DevPipeline &dp = (materialize && !sh.flat) ? p->host_mat : p->host_count;
	sh.dp = &dp;
	sh.wq = dp.W + (dp.mult ? 1u : 0u);
	sh.wpb = sh.flat ? p->flat_wpb : polr_pool_waves_per_block(dp.k, sh.wq);
	// a fused GROUP BY sink keeps its cells in the workgroup's LDS when they fit behind the bit tables, the queues and
	// the router areas (160 KB per workgroup), else in its table in global memory.  (Decided BEFORE the grid is sized:
	// the workgroups per CU are those of the launch as it is made -- a workgroup that is not co-resident would take
	// its routers' executors with it.)
	sh.fused_words = 0;
	if (sh.flat && sh.wpb && out && out->fused_dev) {
		const uint64_t words = (uint64_t)out->fused_groups * polr_fused_group_words(out->fused_aggs);
		if (polr_pool_flat_lds_bytes(dp.k, sh.wpb, dp.lds_table_dwords) + 8 + words * 8 <= 160u * 1024u) {
			sh.fused_words = (uint32_t)words;
		}
	}
	sh.occ = sh.wpb == 0 ? 0
	                     : (sh.flat ? polr_pool_flat_occupancy(dp.k, sh.wpb, dp.lds_table_dwords, materialize, sh.fused_words)
	                                : polr_pool_occupancy(dp.k, sh.wq, dp.ext != 0, agg_sink));
	sh.router_areas = sh.flat && sh.occ >= 1 ? polr_pool_flat_router_areas(dp.k, sh.wpb, dp.lds_table_dwords) : 0u;
	return sh;
}

int polr_pipeline_launch_info(polr_pipeline *p, int materialize, polr_launch_info *info) {
	POLR_ENTRY();
	if (!p || !info) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = p->ctx;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const PoolShape sh = pool_shape(p, materialize != 0, nullptr); // (the occupancy without a fused sink's cells)
	const DevPipeline &dp = *sh.dp;
	memset(info, 0, sizeof(*info));
	info->waves_per_workgroup = sh.wpb;
	if (sh.occ < 1) {
		POLR_FAIL(ctx, POLR_E_UNSUPPORTED, "per-wave LDS queues exceed 160 KB (too many joins x carried ids)");
	}
	info->workgroups_per_cu = (uint32_t)std::min(sh.occ, 8);
	info->lds_bytes_per_workgroup = (uint32_t)(sh.flat ? polr_pool_flat_lds_bytes(dp.k, sh.wpb, dp.lds_table_dwords)
	                                                   : polr_pool_lds_bytes(dp.k, sh.wq));
	info->compiled_stages = dp.k <= 2 ? 2 : (dp.k <= 4 ? 4 : (dp.k <= 6 ? 6 : 8));
	info->tuple_slots = sh.flat ? dp.W : sh.wq;
	info->n_cus = (uint32_t)ctx->n_cus;
	info->flat = sh.flat ? 1u : 0u;
	info->lds_tables = sh.flat ? dp.n_lds_tables : 0u;
	info->lds_table_bytes = sh.flat ? dp.lds_table_dwords * 4u : 0u;
	return POLR_OK;
}

// the source chunks are the ones polr_pipeline_scan_filter produced (boundaries stay on the device)
int polr_mpx_use_scan_chunks(polr_mpx *m) {
	POLR_ENTRY();
	if (!m) {
		return POLR_E_INVALID;
	}
	polr_pipeline *p = m->pipe;
	polr_ctx *ctx = p->ctx;
	if (!p->scan_valid) {
		POLR_FAIL(ctx, POLR_E_INVALID, "no scan result: call polr_pipeline_scan_filter first");
	}
	if (m->chunk_offsets_own) {
		HIPCHK(ctx, hipSetDevice(ctx->device));
		m->chunk_offsets_own.reset();
	}
	m->chunk_offsets_dev = p->scan_offsets_dev;
	m->from_scan = true;
	m->scan_generation = p->scan_generation;
	m->n_chunks = p->scan_n_chunks;
	return POLR_OK;
}

// ---- a run = begin (set range, prime the first round) + a non-blocking pump that keeps a few
// self-routing launches queued ahead of the progress the device publishes -------------------------
struct RunState {
	polr_mpx *m = nullptr;
	hipStream_t st = nullptr;
	SelfRoute sr;
	DevOut dout;
	const DevPipeline *dpd = nullptr;
	uint32_t W = 0, k = 0, max_blocks = 0, wpb = 0;
	uint32_t launched = 0, base_steps = 0;
	bool finished = false;
};

static int run_begin(RunState &rs, polr_mpx *m, void *stream, uint64_t chunk_begin, uint64_t chunk_end,
                     polr_out *out, uint32_t share) {
	polr_pipeline *p = m->pipe;
	polr_ctx *ctx = p->ctx;
	if (m->from_scan && (!p->scan_valid || m->scan_generation != p->scan_generation)) {
		POLR_FAIL(ctx, POLR_E_INVALID, "the pipeline was scanned again: call polr_mpx_use_scan_chunks");
	}
	if (chunk_begin > chunk_end || chunk_end > m->n_chunks) {
		POLR_FAIL(ctx, POLR_E_INVALID, "chunks [%llu, %llu) outside the %llu source chunks",
		          (unsigned long long)chunk_begin, (unsigned long long)chunk_end, (unsigned long long)m->n_chunks);
	}
	if (out && out->pipe != p) {
		POLR_FAIL(ctx, POLR_E_INVALID, "output object belongs to another pipeline");
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = stream ? (hipStream_t)stream : m->own_stream;
	HIPCHK(ctx, adopt_stream(m, st));
	const bool materialize = out != nullptr;
	uint32_t unit_unused, max_blocks;
	int rc = polr_plan_launch(p, materialize, p->n_tuples, &unit_unused, &max_blocks);
	if (rc) {
		return rc;
	}
#ifdef POLR_DIAG_STAMPS
	if (!m->stamps_dev) {
		HIPCHK(ctx, m->stamps_dev.alloc(4096 * 8));
		HIPCHK(ctx, hipMemset(m->stamps_dev, 0, 4096 * 8 * 8));
	}
#endif
	// executors that run concurrently share the device: each sizes its units and grid for its share
	uint32_t resident_waves = std::max<uint32_t>(polr_resident_waves(p, materialize) / std::max<uint32_t>(share, 1), 256);
	const uint32_t wpb = polr_waves_per_block(p, materialize);
	max_blocks = std::max<uint32_t>(max_blocks / std::max<uint32_t>(share, 1), 64);
	rs.m = m;
	rs.st = st;
	m->stats_in_host = false;
	memset(&rs.dout, 0, sizeof(rs.dout));
	if (out) {
		rs.dout = out->dev;
		out->stats_valid = false;
		HIPCHK(ctx, out_order_behind_reset(out, st));
	}
	const DevPipeline &dp = materialize ? p->host_mat : p->host_count;
	rs.dpd = materialize ? p->dev_mat : p->dev_count;
	rs.W = dp.W;
	rs.k = dp.k;
	rs.max_blocks = max_blocks;
	rs.wpb = wpb;
	if (m->pending_sync) { // a previous run left launches queued: settle before reading progress
		HIPCHK(ctx, hipStreamSynchronize(st));
		m->pending_sync = false;
	}
	hipLaunchKernelGGL(polr_mpx_set_range_kernel, dim3(1), dim3(1), 0, st, m->dev, chunk_begin, chunk_end,
	                   (const uint64_t *)m->chunk_offsets_dev, m->n_chunks, p->n_tuples);
	m->steps_base = m->done_host[POLR_HW_STEPS];
	m->done_host[POLR_HW_DONE] = 0;
	m->steal_run = false;
	// prime: route the first round of this run into the descriptor slot the next launch reads
	const uint32_t slot0 = m->iter & 1u;
	hipLaunchKernelGGL(polr_mpx_router_kernel, dim3(1), dim3(64), 0, st, m->dev, m->round_dev + slot0,
	                   m->prefix_dev + 2 * slot0, m->unit_size_dev + slot0, m->counts_dev, p->k, resident_waves);
	rs.sr.mpx = m->dev;
	rs.sr.rounds_base = m->round_dev;
	rs.sr.prefix_base = m->prefix_dev;
	rs.sr.unit_base = m->unit_size_dev;
	rs.sr.ticket = m->ticket_dev;
	rs.sr.resident_waves = resident_waves;
	rs.sr.stamps = m->stamps_dev;
	rs.sr.iter = 0;
	rs.launched = 0;
	rs.base_steps = m->steps_base;
	rs.finished = false;
	m->last_stream = st;
	return POLR_OK;
}

// Every launch probes the round in its slot and its last workgroup routes the next one.  The host never
// synchronises inside a run: it keeps a few launches queued ahead of the progress the device publishes
// (pinned host words written by the router) and stops when the router reports the end of the range.
// Launches queued past the end find an empty round and exit.  Non-blocking: returns after at most one launch.
static int run_pump(RunState &rs) {
	polr_mpx *m = rs.m;
	polr_ctx *ctx = m->pipe->ctx;
	const uint32_t look_ahead = 3;
	const uint32_t steps = m->done_host[POLR_HW_STEPS] - rs.base_steps; // 1 after the prime step, +1 per routed launch
	if (m->done_host[POLR_HW_DONE] && steps >= 1) {
		rs.finished = true; // the router has seen the end of the range
		m->steps_base = m->done_host[POLR_HW_STEPS];
		m->pending_sync = true; // the queued tail is drained by whoever synchronises next
		return POLR_OK;
	}
	if (rs.launched + 1 > steps + look_ahead) {
		return POLR_OK; // enough launches in flight
	}
	size_t ev = 0;
	int rc = timing_start(m, rs.st, &ev);
	if (rc) {
		return rc;
	}
	rs.sr.iter = m->iter++;
	hipError_t e = polr_launch_path_kernel(rs.W, rs.k, rs.max_blocks, rs.wpb, rs.st, rs.dpd, m->round_dev,
	                                       m->prefix_dev, 1, m->unit_size_dev, rs.dout, m->counts_dev, rs.sr);
	if (e != hipSuccess) {
		POLR_FAIL(ctx, POLR_E_HIP, "path kernel launch failed: %s", hipGetErrorString(e));
	}
	rs.launched++;
	return timing_stop(m, rs.st, ev);
}

int polr_mpx_run(polr_mpx *m, void *stream, uint64_t chunk_begin, uint64_t chunk_end, polr_out *out) {
	POLR_ENTRY();
	if (!m) {
		return POLR_E_INVALID;
	}
	POLR_REFUSE_FUSED(m->pipe->ctx, out);
	RunState rs;
	int rc = run_begin(rs, m, stream, chunk_begin, chunk_end, out, 1);
	while (!rc && !rs.finished) {
		rc = run_pump(rs);
	}
	return rc;
}

// Several executors at once (the reference runs one PipelineExecutor + MultiplexerState per worker
// thread over morsels of one pipeline, pipeline.cpp:145-174): every multiplexer routes its own chunk
// range on its own stream; one host thread pumps them round-robin, so their routing rounds overlap on
// the device instead of queueing behind each other.
int polr_mpx_run_many(polr_mpx **ms, void **streams, const uint64_t *chunk_begin, const uint64_t *chunk_end,
                      uint32_t n, polr_out *out) {
	POLR_ENTRY();
	if (!ms || !ms[0] || !chunk_begin || !chunk_end || n == 0) {
		return POLR_E_INVALID;
	}
	POLR_REFUSE_FUSED(ms[0]->pipe->ctx, out);
	std::vector<RunState> rs(n);
	int rc = POLR_OK;
	for (uint32_t i = 0; i < n && !rc; i++) {
		if (!ms[i] || ms[i]->pipe != ms[0]->pipe) {
			return POLR_E_INVALID;
		}
		rc = run_begin(rs[i], ms[i], streams ? streams[i] : nullptr, chunk_begin[i], chunk_end[i], out, n);
	}
	bool all_done = false;
	while (!rc && !all_done) {
		all_done = true;
		for (uint32_t i = 0; i < n && !rc; i++) {
			if (!rs[i].finished) {
				rc = run_pump(rs[i]);
				all_done = all_done && rs[i].finished;
			}
		}
	}
	return rc;
}

// The whole run in ONE launch (polr_pool.hip): one router wave per executor + a pool of probe waves that serves
// the rounds of all executors; routing decisions never leave the device, the host only enqueues.  Asynchronous:
// polr_mpx_finish / _finish_many synchronise.
//
// run_resident_impl prepares it in phases: validate the request, the launch's shape (pool_shape), its plan
// (polr_pool_plan.h), the device buffers, the descriptors, enqueue.  Every refusal (POLR_E_INVALID /
// POLR_E_UNSUPPORTED: validate_request, plan_run) happens before the first change to any multiplexer's state and
// before anything is enqueued.

// where the executors of a run get their chunks from, and how the run is made (filled by the five entry points)
struct ResidentRequest {
	const uint64_t *range_begin, *range_end; // [n][ranges_per_exec]: executor i routes its ranges in order (unless morsels)
	uint32_t ranges_per_exec;
	uint64_t morsel_begin, morsel_end; // morsel_chunks != 0: the executors share these chunks, pulled from one cursor
	uint32_t morsel_chunks;
	bool backpressure;     // executor i sends everything down join order i
	uint32_t grant_chunks; // != 0: range stealing, chunks per grant
	uint32_t flags;
	polr_out *out;
};

// executor i routes the ranges_per_exec ranges [i][..] of begin / end, in order
static ResidentRequest ranges_request(const uint64_t *begin, const uint64_t *end, uint32_t ranges_per_exec, polr_out *out,
                                      uint32_t flags) {
	ResidentRequest rq = {};
	rq.range_begin = begin;
	rq.range_end = end;
	rq.ranges_per_exec = ranges_per_exec;
	rq.out = out;
	rq.flags = flags;
	return rq;
}

// the executors share the chunks [begin, end) and pull them morsel_chunks at a time
static ResidentRequest morsel_request(uint64_t begin, uint64_t end, uint32_t morsel_chunks, polr_out *out, uint32_t flags) {
	ResidentRequest rq = {};
	rq.ranges_per_exec = 1;
	rq.morsel_begin = begin;
	rq.morsel_end = end;
	rq.morsel_chunks = morsel_chunks;
	rq.out = out;
	rq.flags = flags;
	return rq;
}

#define POOL_HEADER_BYTES 512
static_assert(sizeof(PoolRun) <= POOL_HEADER_BYTES, "run header");

static int validate_request(polr_mpx **ms, uint32_t n, const ResidentRequest &rq) {
	if (!ms || n == 0 || !ms[0] || (rq.morsel_chunks == 0 && (!rq.range_begin || !rq.range_end))) {
		return POLR_E_INVALID;
	}
	polr_pipeline *p = ms[0]->pipe;
	polr_ctx *ctx = p->ctx;
	if (n > 4096) {
		POLR_FAIL(ctx, POLR_E_UNSUPPORTED, "at most 4096 executors per run");
	}
	if (p->n_tuples >= 0xFFFFFFF0ull) {
		POLR_FAIL(ctx, POLR_E_UNSUPPORTED, "source partition too large for 32-bit tuple positions");
	}
	if (rq.out && rq.out->pipe != p) {
		POLR_FAIL(ctx, POLR_E_INVALID, "output object belongs to another pipeline");
	}
	for (uint32_t i = 0; i < n; i++) {
		if (!ms[i] || ms[i]->pipe != p) {
			return POLR_E_INVALID;
		}
		if (ms[i]->from_scan && (!p->scan_valid || ms[i]->scan_generation != p->scan_generation)) {
			POLR_FAIL(ctx, POLR_E_INVALID, "the pipeline was scanned again: call polr_mpx_use_scan_chunks");
		}
		for (uint32_t r = 0; r < (rq.morsel_chunks ? 1u : rq.ranges_per_exec); r++) {
			const uint64_t cb = rq.morsel_chunks ? rq.morsel_begin : rq.range_begin[(size_t)i * rq.ranges_per_exec + r];
			const uint64_t ce = rq.morsel_chunks ? rq.morsel_end : rq.range_end[(size_t)i * rq.ranges_per_exec + r];
			if (cb > ce || ce > ms[i]->n_chunks) {
				POLR_FAIL(ctx, POLR_E_INVALID, "chunks [%llu, %llu) outside the %llu source chunks", (unsigned long long)cb,
				          (unsigned long long)ce, (unsigned long long)ms[i]->n_chunks);
			}
		}
	}
	if (rq.grant_chunks) {
		// range stealing rests on the words describing pairwise disjoint pieces of the table (polr_steal.h)
		std::vector<std::pair<uint64_t, uint64_t>> pieces;
		for (uint32_t i = 0; i < n; i++) {
			if (rq.range_begin[i] < rq.range_end[i]) {
				pieces.emplace_back(rq.range_begin[i], rq.range_end[i]);
			}
		}
		std::sort(pieces.begin(), pieces.end());
		for (size_t i = 1; i < pieces.size(); i++) {
			if (pieces[i].first < pieces[i - 1].second) {
				POLR_FAIL(ctx, POLR_E_INVALID, "range stealing needs pairwise disjoint ranges: chunks [%llu, %llu) and [%llu, %llu) overlap",
				          (unsigned long long)pieces[i - 1].first, (unsigned long long)pieces[i - 1].second,
				          (unsigned long long)pieces[i].first, (unsigned long long)pieces[i].second);
			}
		}
	}
	std::vector<polr_mpx *> sorted(ms, ms + n);
	std::sort(sorted.begin(), sorted.end());
	if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) {
		POLR_FAIL(ctx, POLR_E_INVALID, "the same multiplexer twice in one run");
	}
	return POLR_OK;
}

// the plan of a launch of shape `sh` for n executors, and the share of the device it is sized for; refuses what does
// not fit on a CU, a share beyond 16 and more executors than fit on the device
static int plan_run(polr_ctx *ctx, const PoolShape &sh, uint32_t n, uint64_t n_tuples, uint32_t flags, uint32_t *share,
                    PoolPlan *plan) {
	if (sh.occ < 1) {
		POLR_FAIL(ctx, POLR_E_UNSUPPORTED, "pool kernel does not fit on a CU (per-wave LDS queues: too many joins x carried ids)");
	}
	*share = std::max<uint32_t>((flags >> 8) & 0xFFu, 1u);
	if (ctx->tuning.device_share) { // (polr_ctx_set_pool_tuning)
		*share = ctx->tuning.device_share;
	}
	if (*share > 16) {
		POLR_FAIL(ctx, POLR_E_INVALID, "device share 1/%u: at most 16 runs side by side", *share);
	}
	*plan = polr_pool_plan((uint32_t)ctx->n_cus, sh.occ, *share, sh.flat, sh.wq, sh.wpb, sh.router_areas, n, n_tuples,
	                       ctx->tuning);
	if (!plan->fits) {
		POLR_FAIL(ctx, POLR_E_UNSUPPORTED, "%u executors do not fit on the device at once", n);
	}
	return POLR_OK;
}

// the buffers of the runs `m0` leads, large enough for this one: descriptors, work-sharing records, unit rings, claim words
static int ensure_run_buffers(polr_mpx *m0, hipStream_t st, uint32_t n, const PoolPlan &pl, bool stealing) {
	polr_ctx *ctx = m0->pipe->ctx;
	// (growing: what is queued on st may still use the old buffer, so the stream is synchronised before ensure frees it)
	if (!m0->execs_dev || m0->execs_cap < n) {
		const uint32_t cap = std::max<uint32_t>(n, 8);
		m0->execs_host.clear();
		if (m0->execs_dev) {
			HIPCHK(ctx, hipStreamSynchronize(st));
		}
		HIPCHK(ctx, m0->execs_dev.ensure(POOL_HEADER_BYTES + (size_t)cap * sizeof(ResidentExec) + 64));
		m0->execs_cap = cap;
	}
	if (m0->done_host[POLR_HW_GIVEN_UP]) {
		// an earlier run on these rings was given up (whoever finished it): probe waves left holding tickets
		m0->pool_dirty = true;
		if (!m0->pending_sync) {
			m0->done_host[POLR_HW_GIVEN_UP] = 0; // (nothing in flight that could still report it)
		}
	}
	// work-sharing records, one per probe wave, and their flags: all flags are 0 between runs (a record is released by the
	// wave that took it) unless a run was given up
	if (pl.share_after != 0xFFFFFFFFu) {
		const size_t need = ((size_t)pl.pool_waves * pl.share_stride + pl.pool_waves) * sizeof(uint32_t);
		if (!m0->share_dev || m0->share_dev.bytes() < need) {
			if (m0->share_dev) {
				HIPCHK(ctx, hipStreamSynchronize(st));
			}
			HIPCHK(ctx, m0->share_dev.ensure(need / sizeof(uint32_t)));
			HIPCHK(ctx, hipMemsetAsync(m0->share_dev, 0, need, st));
		} else if (m0->pool_dirty) {
			HIPCHK(ctx, hipMemsetAsync(m0->share_dev, 0, m0->share_dev.bytes(), st));
		}
	}
	// unit rings: never smaller than before; zeroed when new or when a run on them was given up
	const bool too_small = m0->pool_lo_cap < pl.lo_cap || m0->pool_hi_cap < pl.hi_cap;
	if (!m0->pool_dev || too_small || m0->pool_dirty) {
		const uint32_t lc = std::max(pl.lo_cap, m0->pool_lo_cap), hc = std::max(pl.hi_cap, m0->pool_hi_cap);
		const size_t bytes = sizeof(PoolSync) + (size_t)POLR_POOL_RINGS * (2 * (size_t)lc + hc) * sizeof(PoolEntry);
		if (!m0->pool_dev || too_small) {
			if (m0->pool_dev) {
				HIPCHK(ctx, hipStreamSynchronize(st));
			}
			HIPCHK(ctx, m0->pool_dev.ensure(bytes));
		}
		HIPCHK(ctx, hipMemsetAsync(m0->pool_dev, 0, bytes, st));
		m0->pool_lo_cap = lc;
		m0->pool_hi_cap = hc;
		m0->pool_dirty = false;
	}
	if (stealing && m0->steal_dev.size() < (uint64_t)n * 5) {
		if (m0->steal_dev) {
			HIPCHK(ctx, hipStreamSynchronize(st));
		}
		HIPCHK(ctx, m0->steal_dev.ensure((uint64_t)std::max<uint32_t>(n, 8) * 5));
	}
	return POLR_OK;
}

// where the morsel cursor of the runs `m0` leads sits: behind the executor descriptors
static unsigned long long *morsel_cursor_dev(polr_mpx *m0) {
	return (unsigned long long *)(m0->execs_dev + POOL_HEADER_BYTES + (size_t)m0->execs_cap * sizeof(ResidentExec));
}

// the run header (from the plan) and the executor descriptors (from the request), as they go to the device; marks the
// multiplexers as taking part in this run
static std::vector<char> fill_descriptors(polr_mpx **ms, uint32_t n, const ResidentRequest &rq, const PoolPlan &pl) {
	polr_mpx *m0 = ms[0];
	std::vector<char> host(POOL_HEADER_BYTES + (size_t)n * sizeof(ResidentExec), 0);
	PoolRun *hr = (PoolRun *)host.data();
	ResidentExec *ex = (ResidentExec *)(host.data() + POOL_HEADER_BYTES);
	const bool sharing = pl.share_after != 0xFFFFFFFFu;
	hr->sync = (PoolSync *)m0->pool_dev.get();
	hr->n_exec = n;
	hr->n_router_blocks = pl.n_router_blocks;
	hr->routers_per_block = pl.routers_per_block;
	hr->routers_rem = pl.routers_rem;
	hr->n_rings = pl.n_rings;
	hr->units_x = pl.units_x;
	hr->hi_lottery = pl.hi_lottery;
	hr->hi_unit = pl.hi_unit;
	memcpy(hr->worker_waves, pl.worker_waves, sizeof(hr->worker_waves));
	hr->pool_waves = pl.pool_waves;
	hr->lo_cap = m0->pool_lo_cap; // (the rings as they are: never smaller than the plan's)
	hr->hi_cap = m0->pool_hi_cap;
	hr->hi_tuples = pl.hi_tuples;
	hr->idle_sleep = pl.idle_sleep;
	hr->timeout_ticks = pl.timeout_ticks;
	hr->share_recs = sharing ? m0->share_dev : nullptr;
	hr->share_flags = sharing ? m0->share_dev + (size_t)pl.pool_waves * pl.share_stride : nullptr;
	hr->share_stride = pl.share_stride;
	hr->share_after = pl.share_after;
	hr->routers_done = 0;
	hr->abort = 0;
	// the rings belong to the multiplexer that leads the run: a run that is given up says so in ITS host words too,
	// whichever router saw the watchdog fire (the leader's own router may have finished long before)
	hr->host_words = m0->progress_dev;
	const uint32_t rpe = rq.ranges_per_exec;
	for (uint32_t i = 0; i < n; i++) {
		polr_mpx *m = ms[i];
		m->leader = m0;
		ex[i].mpx = m->dev;
		ex[i].sync = m->sync_dev;
		ex[i].counts = m->counts_dev;
		if (rq.morsel_chunks) {
			ex[i].morsel_cursor = morsel_cursor_dev(m0);
		} else {
			ex[i].chunk_begin = rq.range_begin[(size_t)i * rpe];
			ex[i].chunk_end = rq.range_end[(size_t)i * rpe];
			ex[i].n_more = rpe - 1;
			for (uint32_t r = 1; r < rpe; r++) {
				ex[i].more_begin[r - 1] = rq.range_begin[(size_t)i * rpe + r];
				ex[i].more_end[r - 1] = rq.range_end[(size_t)i * rpe + r];
			}
		}
		ex[i].morsel_end = rq.morsel_end;
		ex[i].morsel_chunks = rq.morsel_chunks;
		ex[i].path_plus1 = rq.backpressure ? i + 1 : 0;
		ex[i].steal_words = rq.grant_chunks ? m0->steal_dev : nullptr;
		ex[i].grant_chunks = rq.grant_chunks;
		m->steal_run = rq.grant_chunks != 0;
		ex[i].chunk_offsets = m->chunk_offsets_dev;
		ex[i].n_chunks = m->n_chunks;
		ex[i].n_tuples = m->pipe->n_tuples;
		ex[i].flags = rq.flags;
		ex[i].stats_out = m->stats_host_dev;
		m->stats_in_host = (rq.flags & POLR_RUN_FINISH) != 0;
		m->done_host[POLR_HW_DONE] = 0;
	}
	return host;
}

// everything that goes onto the stream: the descriptors, what the device consumes with every launch, the launch
static int enqueue_run(polr_mpx **ms, hipStream_t st, uint32_t n, const ResidentRequest &rq, const PoolShape &sh,
                       const PoolPlan &pl, uint32_t share, const std::vector<char> &host) {
	polr_mpx *m0 = ms[0];
	polr_pipeline *p = m0->pipe;
	polr_ctx *ctx = p->ctx;
	// A pass that repeats the previous one (same executors, ranges, flags: every step of a measurement loop) finds its
	// descriptors on the device already; only the two words the device writes (routers_done, abort) are cleared.
	// Otherwise: one copy (pageable source: staged by the runtime before the call returns).
	if (m0->execs_host == host) {
		static_assert(offsetof(PoolRun, abort) == offsetof(PoolRun, routers_done) + 4, "cleared together");
		HIPCHK(ctx, hipMemsetAsync(m0->execs_dev + offsetof(PoolRun, routers_done), 0, 8, st));
	} else {
		HIPCHK(ctx, hipMemcpyAsync(m0->execs_dev, host.data(), host.size(), hipMemcpyHostToDevice, st));
		m0->execs_host = host;
	}
	if (rq.morsel_chunks) {
		const unsigned long long first = rq.morsel_begin;
		HIPCHK(ctx, hipMemcpyAsync(morsel_cursor_dev(m0), &first, 8, hipMemcpyHostToDevice, st));
	}
	if (rq.grant_chunks) {
		// the claim words (and the zeroed counters behind them) with EVERY launch: the device consumes them, so a pass
		// that repeats the previous one and re-sends no descriptors still needs them fresh
		m0->steal_host.assign((size_t)n * 5, 0ull);
		for (uint32_t i = 0; i < n; i++) {
			m0->steal_host[i] = polr_steal::pack((uint32_t)rq.range_begin[i], (uint32_t)rq.range_end[i]);
		}
		HIPCHK(ctx, hipMemcpyAsync(m0->steal_dev, m0->steal_host.data(), (size_t)n * 5 * sizeof(unsigned long long),
		                           hipMemcpyHostToDevice, st));
	}
	DevOut dout;
	memset(&dout, 0, sizeof(dout));
	if (rq.out) {
		dout = rq.out->dev;
		rq.out->stats_valid = false;
		HIPCHK(ctx, out_order_behind_reset(rq.out, st));
	}
	// order this launch behind the pool launches of other streams it must not share the device with
	int rc = order_pool_launch(ctx, st, share);
	size_t ev = 0;
	rc = rc ? rc : timing_start(m0, st, &ev);
	if (rc) {
		return rc;
	}
	const bool materialize = rq.out != nullptr;
	const DevPipeline &dp = *sh.dp;
	const ResidentExec *execs_dev = (const ResidentExec *)(m0->execs_dev + POOL_HEADER_BYTES);
	hipError_t e =
	    sh.flat ? polr_launch_pool_flat_kernel(dp.k, pl.n_blocks, sh.wpb, dp.lds_table_dwords, st, p->dev_count, execs_dev,
	                                           (PoolRun *)m0->execs_dev.get(), dout, materialize, sh.fused_words)
	            : polr_launch_pool_kernel(sh.wq, dp.k, pl.n_blocks, st, materialize ? p->dev_mat : p->dev_count, execs_dev,
	                                      (PoolRun *)m0->execs_dev.get(), dout, dp.ext != 0);
	if (e != hipSuccess) {
		POLR_FAIL(ctx, POLR_E_HIP, "pool kernel launch failed: %s", hipGetErrorString(e));
	}
	rc = timing_stop(m0, st, ev);
	if (rc) {
		return rc;
	}
	HIPCHK(ctx, hipEventRecord(ctx->pool_launches.back().done, st)); // (the entry order_pool_launch made for this launch)
	for (uint32_t i = 0; i < n; i++) {
		ms[i]->pending_sync = true;
	}
	return POLR_OK;
}

static int run_resident_impl(polr_mpx **ms, void *stream, uint32_t n, const ResidentRequest &rq) {
	int rc = validate_request(ms, n, rq);
	if (rc) {
		return rc;
	}
	polr_mpx *m0 = ms[0];
	polr_pipeline *p = m0->pipe;
	polr_ctx *ctx = p->ctx;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const PoolShape sh = pool_shape(p, rq.out != nullptr, rq.out);
	uint32_t share;
	PoolPlan pl;
	rc = plan_run(ctx, sh, n, p->n_tuples, rq.flags, &share, &pl);
	if (rc) {
		return rc;
	}
	// (nothing is refused from here on: the multiplexers' state changes and work is enqueued)
	hipStream_t st = stream ? (hipStream_t)stream : m0->own_stream;
	for (uint32_t i = 0; i < n; i++) {
		// (work still queued on `st` needs no host synchronisation: everything a run touches is ordered by the
		// stream -- consecutive passes can be enqueued back to back)
		HIPCHK(ctx, adopt_stream(ms[i], st));
	}
	rc = ensure_run_buffers(m0, st, n, pl, rq.grant_chunks != 0);
	if (rc) {
		return rc;
	}
	return enqueue_run(ms, st, n, rq, sh, pl, share, fill_descriptors(ms, n, rq, pl));
}

// what run_resident_impl would plan for (ms, n, out, flags), through the same calls; nothing is launched or changed
int polr_mpx_pool_info(polr_mpx **ms, uint32_t n, polr_out *out, uint32_t flags, polr_pool_info *info) {
	POLR_ENTRY();
	if (!ms || n == 0 || !ms[0] || !info) {
		return POLR_E_INVALID;
	}
	polr_pipeline *p = ms[0]->pipe;
	polr_ctx *ctx = p->ctx;
	if (n > 4096) {
		POLR_FAIL(ctx, POLR_E_UNSUPPORTED, "at most 4096 executors per run");
	}
	if (out && out->pipe != p) {
		POLR_FAIL(ctx, POLR_E_INVALID, "output object belongs to another pipeline");
	}
	for (uint32_t i = 0; i < n; i++) {
		if (!ms[i] || ms[i]->pipe != p) {
			return POLR_E_INVALID;
		}
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const PoolShape sh = pool_shape(p, out != nullptr, out);
	uint32_t share;
	PoolPlan pl;
	const int rc = plan_run(ctx, sh, n, p->n_tuples, flags, &share, &pl);
	if (rc) {
		return rc;
	}
	memset(info, 0, sizeof(*info));
	info->n_blocks = pl.n_blocks;
	info->pool_waves = pl.pool_waves;
	info->n_rings = pl.n_rings;
	info->mixed = pl.mixed ? 1u : 0u;
	info->share = share;
	info->units_x = pl.units_x;
	info->hi_unit = pl.hi_unit;
	info->hi_tuples = pl.hi_tuples;
	info->gran = sh.flat ? POLR_POOL_GRAN_FLAT : POLR_POOL_GRAN_GENERIC;
	info->flat = sh.flat ? 1u : 0u;
	return POLR_OK;
}

int polr_mpx_run_resident_ranges(polr_mpx **ms, void *stream, const uint64_t *range_begin, const uint64_t *range_end,
                                 uint32_t ranges_per_executor, uint32_t n, polr_out *out, uint32_t flags) {
	POLR_ENTRY();
	if (ranges_per_executor < 1 || ranges_per_executor > POLR_MORE_RANGES + 1) {
		return POLR_E_INVALID;
	}
	return run_resident_impl(ms, stream, n, ranges_request(range_begin, range_end, ranges_per_executor, out, flags));
}

int polr_mpx_run_resident(polr_mpx **ms, void *stream, const uint64_t *chunk_begin, const uint64_t *chunk_end,
                          uint32_t n, polr_out *out, uint32_t flags) {
	POLR_ENTRY();
	return run_resident_impl(ms, stream, n, ranges_request(chunk_begin, chunk_end, 1, out, flags));
}

// Range stealing (protocol: polr_steal.h; router side: polr_pool_steal_pull).  Every executor routes its own contiguous
// range grant by grant; one that has run dry takes the far half of whoever has most left and goes on there with the
// multiplexer state it has.
// Deterministic: the row set, COUNT(*) and the routed tuples -- every chunk of the ranges is routed exactly once.
// Not deterministic once a steal has happened: which executor routes which chunks, hence per-executor traces and the
// total intermediates (as with morsels, and as in the multi-threaded reference).
// Reproducible all the same: while no executor has two grants to give (grant_chunks >= half of every range) nobody can
// steal, and the run IS the fixed-range run of polr_mpx_run_resident, decision for decision.
int polr_mpx_run_resident_stealing(polr_mpx **ms, void *stream, const uint64_t *chunk_begin, const uint64_t *chunk_end,
                                   uint32_t grant_chunks, uint32_t n, polr_out *out, uint32_t flags) {
	POLR_ENTRY();
	if (!ms || n == 0 || !ms[0] || !chunk_begin || !chunk_end) {
		return POLR_E_INVALID;
	}
	if (grant_chunks == 0) {
		POLR_FAIL(ms[0]->pipe->ctx, POLR_E_INVALID, "range stealing needs a grant of at least one chunk");
	}
	ResidentRequest rq = ranges_request(chunk_begin, chunk_end, 1, out, flags);
	rq.grant_chunks = grant_chunks;
	return run_resident_impl(ms, stream, n, rq);
}

int polr_mpx_steal_stats(polr_mpx *m, polr_steal_stats *stats) {
	POLR_ENTRY();
	if (!m || !stats) {
		return POLR_E_INVALID;
	}
	*stats = m->steal_stats;
	return POLR_OK;
}

int polr_mpx_run_resident_morsels(polr_mpx **ms, void *stream, uint64_t chunk_begin, uint64_t chunk_end,
                                  uint32_t morsel_chunks, uint32_t n, polr_out *out, uint32_t flags) {
	POLR_ENTRY();
	if (morsel_chunks == 0) {
		return POLR_E_INVALID;
	}
	return run_resident_impl(ms, stream, n, morsel_request(chunk_begin, chunk_end, morsel_chunks, out, flags));
}

// BACKPRESSURE routing (MultiplexerRouting::BACKPRESSURE): one executor per join order, all pulling morsels from one
// cursor -- the join orders race for the source (src/parallel/pipeline.cpp:147-156: one PipelineTask per join order
// over ONE shared source state; polar_config.cpp:128-147).  Executor i runs join order i.
int polr_mpx_run_backpressure(polr_mpx **ms, void *stream, uint64_t chunk_begin, uint64_t chunk_end,
                              uint32_t morsel_chunks, polr_out *out, uint32_t flags) {
	POLR_ENTRY();
	if (!ms || !ms[0] || morsel_chunks == 0) {
		return POLR_E_INVALID;
	}
	polr_pipeline *p = ms[0]->pipe;
	polr_ctx *ctx = p->ctx;
	const uint32_t n = p->n_paths;
	for (uint32_t i = 0; i < n; i++) {
		if (!ms[i] || ms[i]->pipe != p) {
			POLR_FAIL(ctx, POLR_E_INVALID, "BACKPRESSURE needs one multiplexer per join order (%u) of the same pipeline", n);
		}
		if (ms[i]->cfg.routing != POLR_ROUTE_BACKPRESSURE && ms[i]->cfg.routing != POLR_ROUTE_DEFAULT_PATH) {
			POLR_FAIL(ctx, POLR_E_INVALID, "multiplexer %u does not route BACKPRESSURE / DEFAULT_PATH", i);
		}
	}
	ResidentRequest rq = morsel_request(chunk_begin, chunk_end, morsel_chunks, out, flags);
	rq.backpressure = true;
	return run_resident_impl(ms, stream, n, rq);
}

int polr_mpx_reset(polr_mpx *m, void *stream) {
	POLR_ENTRY();
	if (!m) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = m->pipe->ctx;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = pick_stream(m, stream);
	HIPCHK(ctx, adopt_stream(m, st));
	if (m->pending_sync) { // launches of the previous pass may still be queued on its stream
		HIPCHK(ctx, hipStreamSynchronize(st));
		m->pending_sync = false;
	}
	m->stats_in_host = false;
	HIPCHK(ctx, hipMemsetAsync(m->counts_dev, 0, POLR_SLOTS * POLR_NSHARD * POLR_KMAX * 8, st));
	hipLaunchKernelGGL(polr_mpx_init_kernel, dim3(1), dim3(1), 0, st, m->dev, m->cfg, m->pipe->n_paths,
	                   m->pipe->n_tuples, m->n_chunks, m->log_path, m->log_tuples, m->log_inter, m->wide0_mask,
	                   m->progress_dev, m->done_host[POLR_HW_STEPS]);
	return POLR_OK;
}

#ifdef POLR_DIAG_STAMPS
// diagnostic: dump the stamps of the first `n` launches (100 MHz ticks)
extern "C" int polr_mpx_dump_stamps(polr_mpx *m, unsigned long long *dst, uint32_t n) {
	return hipMemcpy(dst, m->stamps_dev, (size_t)n * 8 * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif

int polr_mpx_enable_timing(polr_mpx *m, int enable) {
	POLR_ENTRY();
	if (!m) {
		return POLR_E_INVALID;
	}
	m->timing = enable != 0;
	return POLR_OK;
}

int polr_mpx_kernel_time(polr_mpx *m, double *total_ms, uint64_t *n_launches) {
	POLR_ENTRY();
	if (!m || !total_ms || !n_launches) {
		return POLR_E_INVALID;
	}
	*total_ms = m->timed_ms;
	*n_launches = m->timed_launches;
	m->timed_ms = 0;
	m->timed_launches = 0;
	return POLR_OK;
}

// Finishing a run, per multiplexer: enqueue_close, synchronise its stream, settle.
// enqueue_close: the closing kernel and the read-back of its statistics into *stats -- unless the resident run closed
// itself (POLR_RUN_FINISH): nothing to launch
static hipError_t enqueue_close(polr_mpx *m, hipStream_t st, polr_mpx_stats *stats) {
	if (m->stats_in_host) {
		return hipSuccess;
	}
	if (hipError_t e = m->stats_dev.ensure(1)) {
		return e;
	}
	hipLaunchKernelGGL(polr_mpx_finish_kernel, dim3(1), dim3(64), 0, st, m->dev, m->counts_dev, m->pipe->k, m->stats_dev);
	return hipMemcpyAsync(stats, m->stats_dev, sizeof(polr_mpx_stats), hipMemcpyDeviceToHost, st);
}

// settle: after the stream of `m` has been synchronised.  true: its run was given up (the word is read and cleared)
static bool settle(polr_mpx *m, polr_mpx_stats *stats) {
	if (m->stats_in_host) {
		memcpy(stats, m->stats_host, sizeof(polr_mpx_stats));
	}
	m->pending_sync = false;
	collect_steal_stats(m);
	if (m->timing) {
		drain_events(m);
	}
	const bool given_up = m->done_host[POLR_HW_GIVEN_UP] != 0;
	m->done_host[POLR_HW_GIVEN_UP] = 0;
	return given_up;
}

// the rings of a run that was given up are re-initialised before the next one: they belong to the multiplexer that led it
static void mark_rings_dirty(polr_mpx *m) {
	m->pool_dirty = true;
	if (m->leader) {
		m->leader->pool_dirty = true;
	}
}

// whose watchdog fired, and on what: a router that saw it leaves the wait it gave up on in its pinned words; appended to
// `who` (and the words released for the next run)
static void report_watchdog(polr_mpx *m, std::string &who) {
	volatile uint32_t *w = m->done_host;
	if (!w[POLR_HW_DIAG_VALID]) {
		return;
	}
	char buf[200];
	snprintf(buf, sizeof(buf), "%s executor %u: slot %u, %u round(s) in flight, %llu of %llu arrival tokens (65536 per unit)",
	         who.empty() ? ";" : ",", w[POLR_HW_DIAG_EXEC], w[POLR_HW_DIAG_SLOT], w[POLR_HW_DIAG_IN_FLIGHT],
	         ((unsigned long long)w[POLR_HW_DIAG_ARRIVED_HI] << 32) | w[POLR_HW_DIAG_ARRIVED_LO],
	         ((unsigned long long)w[POLR_HW_DIAG_WANTED_HI] << 32) | w[POLR_HW_DIAG_WANTED_LO]);
	who += buf;
	w[POLR_HW_DIAG_VALID] = 0;
}

int polr_mpx_finish(polr_mpx *m, void *stream, polr_mpx_stats *stats) {
	POLR_ENTRY();
	if (!m || !stats) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = m->pipe->ctx;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = pick_stream(m, stream);
	HIPCHK(ctx, adopt_stream(m, st));
	hipError_t e = enqueue_close(m, st, stats);
	e = e == hipSuccess ? hipStreamSynchronize(st) : e;
	if (e != hipSuccess) {
		POLR_FAIL(ctx, POLR_E_HIP, "multiplexer finish failed: %s", hipGetErrorString(e));
	}
	if (settle(m, stats)) {
		mark_rings_dirty(m);
		std::string who;
		report_watchdog(m, who);
		POLR_FAIL(ctx, POLR_E_HIP, "run timed out waiting for its probe waves (results incomplete)%s", who.c_str());
	}
	return POLR_OK;
}

// finish several executors: all closing kernels and read-backs are queued first, then each stream is
// synchronised once (saves n-1 serial round trips)
int polr_mpx_finish_many(polr_mpx **ms, uint32_t n, polr_mpx_stats *stats) {
	POLR_ENTRY();
	if (!ms || !stats || n == 0) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = ms[0]->pipe->ctx;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	for (uint32_t i = 0; i < n; i++) {
		HIPCHK(ctx, enqueue_close(ms[i], pick_stream(ms[i], nullptr), &stats[i]));
	}
	bool timed_out = false;
	hipStream_t synced = nullptr;
	for (uint32_t i = 0; i < n; i++) {
		hipStream_t st = pick_stream(ms[i], nullptr);
		if (st != synced) { // (executors of a resident run share one stream)
			HIPCHK(ctx, hipStreamSynchronize(st));
			synced = st;
		}
		timed_out = settle(ms[i], &stats[i]) || timed_out;
		if (timed_out) { // (and every executor behind the first one that timed out)
			ms[0]->pool_dirty = true;
			mark_rings_dirty(ms[i]);
		}
	}
	if (timed_out) {
		std::string who;
		for (uint32_t i = 0; i < n; i++) {
			report_watchdog(ms[i], who);
		}
		POLR_FAIL(ctx, POLR_E_HIP, "run timed out waiting for its probe waves (results incomplete)%s", who.c_str());
	}
	return POLR_OK;
}

int polr_mpx_fetch_log(polr_mpx *m, void *stream, uint32_t *path, uint64_t *tuples, uint64_t *intermediates,
                       uint64_t max_rounds, uint64_t *n_rounds) {
	POLR_ENTRY();
	if (!m || !n_rounds) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = m->pipe->ctx;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = pick_stream(m, stream);
	DevMpx h;
	HIPCHK(ctx, hipMemcpyAsync(&h, m->dev, sizeof(DevMpx), hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	const uint64_t n = std::min<uint64_t>(h.n_log, max_rounds);
	*n_rounds = n;
	if (n) {
		if (path) {
			HIPCHK(ctx, hipMemcpyAsync(path, m->log_path, n * 4, hipMemcpyDeviceToHost, st));
		}
		if (tuples) {
			HIPCHK(ctx, hipMemcpyAsync(tuples, m->log_tuples, n * 8, hipMemcpyDeviceToHost, st));
		}
		if (intermediates) {
			HIPCHK(ctx, hipMemcpyAsync(intermediates, m->log_inter, n * 8, hipMemcpyDeviceToHost, st));
		}
		HIPCHK(ctx, hipStreamSynchronize(st));
	}
	return POLR_OK;
}

void polr_mpx_destroy(polr_mpx *m) {
	POLR_ENTRY();
	if (!m) {
		return;
	}
	hipSetDevice(m->ctx->device);
	if (m->own_stream) {
		hipStreamSynchronize(m->own_stream);
		hipStreamDestroy(m->own_stream);
	}
	if (m->done_host) {
		hipHostFree((void *)m->done_host);
	}
	if (m->stats_host) {
		hipHostFree(m->stats_host);
	}
	for (auto e : m->ev_start) {
		hipEventDestroy(e);
	}
	for (auto e : m->ev_stop) {
		hipEventDestroy(e);
	}
	polr_ctx *ctx_ = m->ctx;
	delete m;
	polr_ctx_release(ctx_);
}

} // extern "C"
