// duckdb-polr_amd/csrc/polr_internal.h -- host-side objects behind the opaque handles of
// include/polr_hip.h, shared by polr_capi.hip and polr_mpx.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <memory>
#include <string>
#include <vector>

#include "../../include/polr_hip.h"
#include "polr_device.h"
#include "polr_devbuf.h"
#include "polr_mpx_device.h"

// Shared ownership: every object created on a context (build sides, pipelines, outputs, multiplexers) holds a
// reference, so destroying them in any order -- also AFTER polr_ctx_destroy, which a garbage-collected binding does
// routinely -- never reads a freed context (it used to: hipSetDevice(<freed>->device) failed with "invalid device
// ordinal" and left that status in the thread's last-error slot for the next launch check to find).
struct polr_ctx {
	int device = 0;
	hipStream_t stream = nullptr;
	int n_cus = 256;
	std::string err;
	std::atomic<int> refs {1};
	bool closed = false; // polr_ctx_destroy was called: the stream is gone, the object lives on for its children
	polr_pool_tuning tuning {}; // polr_ctx_set_pool_tuning (all zero: defaults)
	// Pool launches in flight (polr_mpx.hip: order_pool_launch).  A pool launch is sized for the whole device -- or for the
	// share of it its flags declare -- and its waves stay on the device until the run is over; two full-size launches on
	// two streams would each hold part of the device with waves that wait for work only the rest of their own grid can
	// unblock, and the watchdog of whichever router waits longest would give its run up.  The library orders them.
	struct PoolLaunch {
		hipStream_t stream;
		hipEvent_t done;
		uint32_t share;
	};
	std::vector<PoolLaunch> pool_launches;
	std::vector<hipEvent_t> pool_events_free;
};

static inline polr_ctx *polr_ctx_retain(polr_ctx *ctx) {
	ctx->refs.fetch_add(1, std::memory_order_relaxed);
	return ctx;
}
static inline void polr_ctx_release(polr_ctx *ctx) {
	if (ctx && ctx->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) {
		delete ctx;
	}
}

// A column on the device.  data / valid are what the kernels read; the library's own copies are held by own_data /
// own_valid, and a caller's device memory (POLR_COL_DEVICE) is a column whose owners are empty.
struct OwnedCol {
	uint8_t *data = nullptr;
	uint8_t *valid = nullptr;
	uint32_t width = 0;
	uint32_t flags = 0;
	bool strings_rebased = false; // string cells point into a device heap (set_string_heaps): a second upload is refused
	DevBuf<uint8_t> own_data, own_valid;
	// cells the library uploaded that polr_ht_filter compacted into the table's one allocation: the owners are empty, but
	// the column still counts as the library's own for the heap-never-came guards (a long cell's pointer may be the host's)
	bool lib_cells = false;
	bool owned() const {
		return own_data.get() != nullptr || lib_cells;
	}
	hipError_t alloc_data(uint64_t bytes) {
		const hipError_t e = own_data.alloc(bytes);
		data = own_data;
		return e;
	}
	hipError_t alloc_valid(uint64_t bytes) {
		const hipError_t e = own_valid.alloc(bytes);
		valid = own_valid;
		return e;
	}
};

// the dictionary of a code column (polr_ht_encode_dictionary, polr_dict.hip): one representative string_t cell per code,
// pointing into the heap the table owns
struct DictCol {
	uint32_t code_col = 0, src_col = 0; // payload columns: the codes, and the VARCHAR column they encode
	uint32_t n_codes = 0, has_null = 0;
	DevBuf<uint4> cells;                // device, [n_codes]
};

struct polr_ht {
	polr_ctx *ctx = nullptr;
	uint32_t n_keys = 0, n_payload = 0;
	KeyPack pack = {}; // composite keys in packed form (finalize_hash decides)
	uint32_t key_flags[POLR_MAX_KEYS] = {}; // POLR_KEY_* per key column (polr_ht_set_key_flags, before finalize)
	uint64_t n_rows_in = 0; // rows as uploaded (build row ids index these)
	uint64_t n_rows = 0;    // rows kept (NULL keys dropped)
	std::vector<OwnedCol> keys, payload;
	DevBuf<DevCol> keys_dev;    // device array [n_keys]
	DevBuf<DevCol> payload_dev; // device array [n_payload] the probe kernel reads (by build id)
	uint32_t kind = KIND_NONE;
	uint32_t key_signed = 0;
	// the slots of a hash table or the bits of a perfect one: one allocation, table and bits (below) are views of it
	DevBuf<uint8_t> table_mem;
	// hash
	void *table = nullptr;
	uint64_t capacity = 0;
	DevBuf<uint32_t> rowids;
	uint32_t sentinel_start = 0, sentinel_count = 0;
	uint64_t max_run = 0;
	// perfect
	int64_t min_value = 0, max_value = 0;
	uint64_t range = 0;
	uint32_t *bits = nullptr;
	DevBuf<uint32_t> idx_row;
	std::vector<OwnedCol> pcols;
	std::vector<DevBuf<uint8_t>> heaps; // string heaps of VARCHAR payload columns (polr_ht_set_payload_heap), owned
	// a table made by polr_ht_from_output: the cells and validity arrays of all its columns in one allocation -- keys and
	// payload are views of it (their own owners are empty, as for a caller's POLR_COL_DEVICE memory)
	DevBuf<uint8_t> col_mem;
	// polr_ht_filter ran: col_mem holds the kept rows of every column and, behind them, the uploaded row number of every
	// build row (filter_rows, n_rows_in entries: polr_ht_fetch_filter_rows) and the copy descriptors
	bool filtered = false;
	uint32_t *filter_rows = nullptr;
	std::vector<DictCol> dicts; // dictionaries of the code columns (polr_ht_encode_dictionary), cells owned
	uint32_t is_dense = 0, has_null = 0;
	uint64_t device_bytes = 0;
};

// the dictionary whose code column / whose VARCHAR source column is column `col` (a payload column of a table, a probe
// column of a pipeline), or nullptr
static inline const DictCol *polr_dict_of_code_col(const std::vector<DictCol> &dicts, uint32_t col) {
	for (const DictCol &d : dicts) {
		if (d.code_col == col) {
			return &d;
		}
	}
	return nullptr;
}
static inline const DictCol *polr_dict_of_src_col(const std::vector<DictCol> &dicts, uint32_t col) {
	for (const DictCol &d : dicts) {
		if (d.src_col == col) {
			return &d;
		}
	}
	return nullptr;
}
static inline const DictCol *polr_dict_of_code_col(const polr_ht *ht, uint32_t col) {
	return polr_dict_of_code_col(ht->dicts, col);
}
static inline const DictCol *polr_dict_of_src_col(const polr_ht *ht, uint32_t col) {
	return polr_dict_of_src_col(ht->dicts, col);
}

struct polr_pipeline {
	polr_ctx *ctx = nullptr;
	uint32_t k = 0, n_paths = 0, n_probe_cols = 0;
	uint64_t n_probe_rows = 0;
	uint64_t n_tuples = 0;
	std::vector<OwnedCol> probe_cols;
	std::vector<DevBuf<uint8_t>> heaps; // string heaps of VARCHAR probe columns (polr_pipeline_set_probe_heap), owned
	DevBuf<DevCol> probe_cols_dev;
	// dictionaries of the code columns polr_pipeline_encode_dictionary appended (polr_dict.hip), cells owned; they point into
	// the heaps above, or into the caller's
	std::vector<DictCol> dicts;
	// a pipeline made by polr_pipeline_from_output: the cells and validity arrays of all its probe columns in one allocation
	// -- probe_cols are views of it (their own owners are empty, lib_cells is set)
	DevBuf<uint8_t> col_mem;
	uint32_t *sel_dev = nullptr; // the selection in use: a view of sel_upload, of scan_sel, or of the caller's device memory
	DevBuf<uint32_t> sel_upload; // a selection uploaded from the host (polr_pipeline_set_selection)
	// result of polr_pipeline_scan_filter: boundaries of the (non-empty) source chunks in selection positions
	DevBuf<uint64_t> scan_offsets_dev;
	uint64_t scan_n_chunks = 0;
	uint32_t scan_vector_size = 0;
	// scan buffers, sized for the worst case and reused by every scan call, whichever entry point it came through
	DevBuf<uint32_t> scan_sel;
	DevBuf<unsigned long long> scan_packed, scan_sums, scan_totals;
	DevBuf<uint8_t> scan_str_tails; // polr_pipeline_scan_filter_str: the VARCHAR constants' bytes beyond 12, re-uploaded per call
	DevBuf<uint8_t> scan_expr_prog; // polr_pipeline_scan_filter_expr: the lowered program, re-uploaded per call
	// one pass bit per table row, ceil(vector size / 64) words per vector: written by the counting pass, read by the
	// writing pass
	DevBuf<unsigned long long> scan_pass_bits;
	bool scan_valid = false;      // a scan result is installed (selection + chunk boundaries)
	uint64_t scan_generation = 0; // bumped by every scan: multiplexers must re-attach (polr_mpx_use_scan_chunks)
	std::vector<polr_ht *> hts;
	DevPipeline host_count, host_mat; // count-only (narrow tuples) and materialising (all ids) variants
	DevBuf<DevPipeline> dev_count, dev_mat;
	DevBuf<StageDesc> stages_count, stages_mat; // [n_paths][POLR_KMAX] each
	DevBuf<FlatStageRec> stages_flat; // flat pipelines: stages_count as the flat pool kernel reads it
	DevBuf<StageExt> stage_ext; // extension records of both variants (those stages that have one)
	int blocks_per_cu_count = 0, blocks_per_cu_mat = 0;       // measured residency of the path kernel
	uint32_t wpb_count = 0, wpb_mat = 0;                      // waves per workgroup (4, or fewer when the LDS queues are wide)
	uint32_t flat_wpb = 0;                                    // flat pipelines: waves per workgroup of the flat pool kernel
	bool flat_emit = false;                                   // ... and every join is a perfect table: emitting runs take it too
	// launch scratch (grown on demand)
	DevBuf<DevRound> rounds_dev;
	DevBuf<uint64_t> prefix_dev;
	DevBuf<uint32_t> unit_sizes_dev;
	DevBuf<unsigned long long> counts_dev;
	DevBuf<unsigned long long> shards_dev; // [rounds][POLR_NSHARD][k] scratch of the path kernel
};

struct polr_out {
	polr_pipeline *pipe = nullptr;
	polr_ctx *ctx = nullptr; // (kept so that destroying the object never has to go through the pipeline)
	DevOut dev; // (ids, chunk_count and cursor are views of the three buffers below)
	DevBuf<uint32_t> ids, chunk_count, cursor;
	DevBuf<uint64_t> chunk_base; // [max_chunks] exclusive prefix, refreshed by stats
	DevBuf<uint64_t> total_dev;
	uint64_t n_rows = 0;
	uint32_t n_chunks = 0;
	bool stats_valid = false;
	// polr_out_reset only enqueues its memsets: a run that writes this output on ANOTHER stream is ordered behind them
	// by this event (out_order_behind_reset); reset_stream: where the last reset was enqueued
	hipEvent_t reset_event = nullptr;
	hipStream_t reset_stream = nullptr;
	// a fused GROUP BY sink (polr_out_fuse_grouped): the device descriptor, its cell tables, and what the result needs
	DevBuf<FusedSink> fused_dev;
	DevBuf<unsigned long long> fused_cells, fused_dropped;
	uint32_t fused_tables = 0, fused_groups = 0, fused_aggs = 0;
	uint32_t fused_fn[8] = {};
	bool fused_has_valid[8] = {};
	// a fused UNGROUPED aggregate sink (polr_out_fuse_aggregate): the device descriptor, its cell tables (the plan's
	// n_tables, and one more where the read-out combines them), and the plan the reset and the result follow
	DevBuf<FusedAggSink> agg_dev;
	DevBuf<unsigned long long> agg_cells;
	PolrFuseAggPlan agg_plan = {};
};

// the output carries a fused sink of either kind: it holds cells, no row ids
static inline bool out_has_fused_sink(const polr_out *o) {
	return o->fused_dev.get() != nullptr || o->agg_dev.get() != nullptr;
}

#define POLR_FAIL(ctx_, code_, ...)                                                                                    \
	do {                                                                                                               \
		char buf_[512];                                                                                                \
		snprintf(buf_, sizeof(buf_), __VA_ARGS__);                                                                     \
		(ctx_)->err = buf_;                                                                                            \
		return (code_);                                                                                                \
	} while (0)

#define HIPCHK(ctx_, call_)                                                                                            \
	do {                                                                                                               \
		hipError_t e_ = (call_);                                                                                       \
		if (e_ != hipSuccess) {                                                                                        \
			POLR_FAIL(ctx_, POLR_E_HIP, "%s failed: %s (%s:%d)", #call_, hipGetErrorString(e_), __FILE__, __LINE__);   \
		}                                                                                                              \
	} while (0)

// return a POLR_E_* code as it is (the callee has set the context's error)
#define POLR_TRY(call_)                                                                                                \
	do {                                                                                                               \
		const int rc_ = (call_);                                                                                       \
		if (rc_) {                                                                                                     \
			return rc_;                                                                                                \
		}                                                                                                              \
	} while (0)

// a refusal of a host plan (polr_build_plan.h: the code returned, the text in plan.err) becomes the context's error
#define POLR_TRY_PLAN(ctx_, plan_, call_)                                                                              \
	do {                                                                                                               \
		const int rc_ = (call_);                                                                                       \
		if (rc_) {                                                                                                     \
			POLR_FAIL(ctx_, rc_, "%s", (plan_).err);                                                                   \
		}                                                                                                              \
	} while (0)

// Diagnostic (POLR_DEBUG_HIP_ERRORS=1 in the environment): every C-ABI entry point reports a HIP error that an
// EARLIER call left in the thread's last-error slot, naming the entry point that ran before -- how a swallowed
// HIP status is tracked down.  Off: one predictable branch.
void polr_trace_stale(const char *where);
#define POLR_ENTRY() polr_trace_stale(__func__)

// what the functions that build a handle hold it in: POLR_FAIL / HIPCHK inside them then destroy the half-built handle, and
// success hands it out with release()
struct HandleDeleter {
	void operator()(polr_ht *ht) const {
		polr_ht_destroy(ht);
	}
	void operator()(polr_pipeline *p) const {
		polr_pipeline_destroy(p);
	}
	void operator()(polr_out *o) const {
		polr_out_destroy(o);
	}
};
template <class T>
using HandleGuard = std::unique_ptr<T, HandleDeleter>;

// the skeleton of a new build side, behind every route to one: the context retained, the counts set, a column record per
// key and payload column
static inline HandleGuard<polr_ht> polr_ht_new(polr_ctx *ctx, uint32_t n_keys, uint32_t n_payload, uint64_t n_rows_in) {
	HandleGuard<polr_ht> ht(new polr_ht());
	ht->ctx = polr_ctx_retain(ctx);
	ht->n_keys = n_keys;
	ht->n_payload = n_payload;
	ht->n_rows_in = n_rows_in;
	ht->keys.resize(n_keys);
	ht->payload.resize(n_payload);
	return ht;
}

static inline hipStream_t polr_stream(polr_ctx *ctx, void *stream) {
	return stream ? (hipStream_t)stream : ctx->stream;
}

// the copy of build column i that the kernels read: a perfect table's re-ordered copy, else the payload as uploaded
static inline const OwnedCol &build_col(const polr_ht *ht, uint32_t i) {
	return ht->kind == KIND_PERFECT ? ht->pcols[i] : ht->payload[i];
}

// slot index mask of a hash table (capacity is a power of two; 0 for a perfect table)
static inline uint64_t ht_mask(const polr_ht *ht) {
	return ht->capacity ? ht->capacity - 1 : 0;
}

static inline DevCol dev_col(const OwnedCol &c) {
	DevCol d;
	d.data = c.data;
	d.valid = c.valid;
	d.width = c.width;
	d.flags = c.flags;
	return d;
}

// a run on stream `st` is about to write output `o`: the last polr_out_reset, if it was enqueued on another stream, comes
// first (without this the reset could land behind the run and wipe the cursor: counters right, no rows)
static inline hipError_t out_order_behind_reset(polr_out *o, hipStream_t st) {
	if (!o || !o->reset_event || o->reset_stream == st) {
		return hipSuccess;
	}
	return hipStreamWaitEvent(st, o->reset_event, 0);
}

// the statistics every reader of an output needs (chunk count, prefix): computed once after a run
static inline int out_ensure_stats(polr_out *o, void *stream) {
	return o->stats_valid ? POLR_OK : polr_out_stats(o, stream, nullptr, nullptr, nullptr);
}

// column (src_join, src_col) of a pipeline's output, as a sink reads it (polr_agg.hip, polr_strheap.hip)
struct OutCol {
	const OwnedCol *col;
	uint32_t slot; // the output's row ids that index it: 0 probe, 1 + j join j
	DevCol dev;
};
// POLR_E_INVALID for a column out of range ("<what> <idx>: ..." in the context's error)
int polr_out_col(polr_pipeline *p, int32_t src_join, uint32_t src_col, OutCol *c, const char *what, uint32_t idx);
// the same column described to the sinks' host plan (polr_agg_plan.h); in range: *c is resolved, as by polr_out_col
PolrAggCol polr_out_describe_col(polr_pipeline *p, int32_t src_join, uint32_t src_col, OutCol *c);
// POLR_OK when the VARCHAR column may be read by a kernel that follows string pointers: rebased onto a device heap, the
// caller's own device memory, or without a non-NULL cell longer than 12 bytes among the output rows (polr_strheap.hip;
// counts on stream st and waits for it); else the refusal below
int check_string_col_on_device(polr_out *o, hipStream_t st, const OutCol &c, const char *what, uint32_t idx);

// Strings leave the device as records (polr_strrec_plan.h), by one path (polr_strheap.hip): entry i of n is the string of
// cell d_cells[d_index ? d_index[i] : i] (device memory), at offs[i] (host memory, as polr_strrec_layout laid them out:
// POLR_STRREC_NONE = no record), `used` bytes in all.  Where they fit the caller's room (polr_strrec_fits) the records are
// written on the device into an arena of exactly `used` bytes and that is copied to str_bytes; waits for the stream.
// d_offs: device memory of n words for the offsets that the caller owns and no longer needs, or NULL (allocated here).
// POLR_E_OVERFLOW where they do not fit: nothing was written, and the context's error is left to the caller, whose
// wording it is.
int polr_fetch_str_records(polr_ctx *ctx, hipStream_t st, const uint4 *d_cells, const uint32_t *d_index, uint64_t n,
                           const uint64_t *offs, uint64_t used, uint64_t n_offsets, uint64_t *d_offs, uint8_t *str_bytes,
                           uint64_t str_cap);

// The refusal of a VARCHAR column the library uploaded whose heap never came, once a non-NULL cell longer than 12 bytes
// turns up among the output rows (check_string_col_on_device of polr_strheap.hip; polr_out_materialize_strings counts such
// cells in its measuring pass): one message for every sink.
#define POLR_FAIL_HEAP_NEVER_CAME(ctx_, what_, idx_, n_long_)                                                          \
	POLR_FAIL(ctx_, POLR_E_INVALID,                                                                                    \
	          "%s %u: %llu output rows hold strings longer than 12 bytes, but the column's heap was never put on the "   \
	          "device (polr_ht_set_payload_heaps / polr_pipeline_set_probe_heaps)",                                      \
	          what_, idx_, (unsigned long long)(n_long_))

// Only the flat pool kernel folds tuples into a fused GROUP BY sink (DevOut::fused).  The entry points that launch the
// per-round path kernel refuse such an output before they enqueue anything: that kernel would write row ids instead and
// leave the group cells empty.  The same holds for the generic pool kernel's ungrouped sink (DevOut::agg).
#define POLR_REFUSE_FUSED(ctx_, out_)                                                                                  \
	do {                                                                                                               \
		if ((out_) && (out_)->fused_dev) {                                                                             \
			POLR_FAIL(ctx_, POLR_E_UNSUPPORTED,                                                                        \
			          "%s: the output has a fused GROUP BY sink, which only the pool launch fills "                     \
			          "(polr_mpx_run_resident*, polr_mpx_run_backpressure)",                                           \
			          __func__);                                                                                       \
		}                                                                                                              \
		if ((out_) && (out_)->agg_dev) {                                                                               \
			POLR_FAIL(ctx_, POLR_E_UNSUPPORTED,                                                                        \
			          "%s: the output has a fused aggregate sink, which only the pool launch fills "                    \
			          "(polr_mpx_run_resident*, polr_mpx_run_backpressure)",                                           \
			          __func__);                                                                                       \
		}                                                                                                              \
	} while (0)

// An output with a fused ungrouped sink holds aggregate cells and no row ids: the calls that read row ids refuse it
#define POLR_REFUSE_AGG_CELLS(ctx_, out_)                                                                              \
	do {                                                                                                               \
		if ((out_)->agg_dev) {                                                                                         \
			POLR_FAIL(ctx_, POLR_E_INVALID, POLR_AGG_CELLS_TEXT);                                                      \
		}                                                                                                              \
	} while (0)

// kernels / launchers implemented in polr_build.hip and polr_probe.hip
size_t polr_path_lds_bytes(uint32_t k, uint32_t W, uint32_t waves_per_block);
int polr_path_occupancy(uint32_t k, uint32_t W, uint32_t waves_per_block);
hipError_t polr_launch_path_kernel(uint32_t W, uint32_t k, uint32_t n_blocks, uint32_t waves_per_block,
                                   hipStream_t stream, const DevPipeline *pipe, const DevRound *rounds,
                                   const uint64_t *unit_prefix, uint32_t n_rounds, const uint32_t *unit_sizes,
                                   DevOut out, unsigned long long *counts, SelfRoute sr);
// the whole run in one launch (polr_pool.hip): routers + a pool of probe waves
struct PoolRun;
uint32_t polr_pool_waves_per_block(uint32_t k, uint32_t W); // 0: does not fit at all
size_t polr_pool_lds_bytes(uint32_t k, uint32_t W);
int polr_pool_occupancy(uint32_t k, uint32_t W, bool ext, bool agg = false); // agg: the build that fills a fused ungrouped sink
hipError_t polr_launch_pool_kernel(uint32_t W, uint32_t k, uint32_t n_blocks, hipStream_t stream, const DevPipeline *pipe,
                                   const ResidentExec *execs, PoolRun *run, DevOut out, bool ext);
size_t polr_pool_flat_lds_bytes(uint32_t k, uint32_t waves_per_block, uint32_t table_dwords);
size_t polr_pool_flat_wave_bytes(uint32_t k);
// routers a probe workgroup of the flat kernel can host in its own LDS (0: only router workgroups)
uint32_t polr_pool_flat_router_areas(uint32_t k, uint32_t waves_per_block, uint32_t table_dwords);
// fused_words: 8-byte cells of a fused sink the launch keeps in LDS (the occupancy of the launch as it is made)
int polr_pool_flat_occupancy(uint32_t k, uint32_t waves_per_block, uint32_t table_dwords, bool emit, uint32_t fused_words = 0);
hipError_t polr_launch_pool_flat_kernel(uint32_t k, uint32_t n_blocks, uint32_t waves_per_block, uint32_t table_dwords,
                                        hipStream_t stream, const DevPipeline *pipe, const ResidentExec *execs,
                                        PoolRun *run, DevOut out, bool emit, uint32_t fused_words);
void polr_launch_gather(hipStream_t stream, DevOut out, const uint64_t *chunk_base, uint32_t n_chunks, uint32_t slot,
                        DevCol src, uint8_t *dst_data, uint8_t *dst_valid);
void polr_launch_compact_ids(hipStream_t stream, DevOut out, const uint64_t *chunk_base, uint32_t n_chunks,
                             uint32_t *dst);
// every cell table of the output's fused ungrouped sink back to "no rows" (polr_agg.hip; o->agg_cells is set)
void polr_launch_fuseagg_fill(hipStream_t st, const polr_out *o);
void polr_launch_reduce_counts(hipStream_t stream, const unsigned long long *src, uint64_t n_rounds, uint32_t k,
                               unsigned long long *dst);
void polr_launch_deserialize_col(hipStream_t st, const uint8_t *rows, uint64_t n_rows, uint32_t row_width, uint32_t col,
                                 uint32_t offset, uint32_t width, uint8_t *dst, uint8_t *dst_valid);
void polr_launch_key_minmax(hipStream_t st, const DevCol *keys_dev, uint32_t n_keys, uint64_t n_rows, uint32_t null_eq,
                            long long *out);
void polr_launch_s16_build(hipStream_t st, const DevCol *keys_dev, uint32_t n_keys, const KeyPack &pack, uint64_t n_rows,
                           uint4 *slots,
                           uint64_t capacity, uint32_t *slot_of_row, uint32_t *cursor, uint32_t *rowids,
                           uint32_t *block_sums, uint32_t *scalars, unsigned long long *n_valid);
void polr_launch_scan_blocksums(hipStream_t st, uint32_t *block_sums, uint32_t n_blocks, uint32_t *total);
void polr_launch_s16_scatter(hipStream_t st, uint64_t n_rows, const uint4 *slots, const uint32_t *slot_of_row,
                             uint32_t *cursor, uint32_t *rowids, uint32_t sentinel_start, uint32_t *sentinel_cursor);
void polr_launch_s16_to_s8(hipStream_t st, const uint4 *slots, uint64_t capacity, const uint32_t *rowids, uint2 *s8);
void polr_launch_pht_mark(hipStream_t st, const DevCol *keys_dev, uint64_t n_rows, int64_t min_value, uint64_t range,
                          uint32_t is_signed, uint32_t *bits, uint32_t *idx_row, uint32_t *flags,
                          unsigned long long *unique_keys);
void polr_launch_pht_gather(hipStream_t st, const uint32_t *bits, const uint32_t *idx_row, uint64_t size, DevCol src,
                            uint8_t *dst, uint8_t *dst_valid);
void polr_launch_pack_bitmap(hipStream_t st, const uint8_t *bytes, uint64_t size, uint32_t *bits);
void polr_launch_chunk_prefix(hipStream_t st, const uint32_t *chunk_count, uint32_t n_chunks, uint64_t *chunk_base,
                              uint64_t *total);
// ... of 64-bit counts (the chunks' heap bytes, polr_strout.hip): the same kernel, nothing truncated
void polr_launch_chunk_prefix(hipStream_t st, const uint64_t *chunk_bytes, uint32_t n_chunks, uint64_t *chunk_base,
                              uint64_t *total);
// the compaction pass of polr_ht_filter (polr_htfilter.hip: polr_htfilter_compact_kernel, a workgroup per tile), n_tiles > 0:
// every column of cols[n_cols] (a device array) and the row list, from the pass bits and the tiles' first output rows
struct PolrHtFilterDesc;
void polr_launch_htfilter_compact(hipStream_t st, const unsigned long long *pass_bits, const uint64_t *tile_base, uint64_t n_tiles,
                                  const PolrHtFilterDesc *cols, uint32_t n_cols, uint32_t *rows);
// the measure and write passes of a VARCHAR output column (polr_strout.hip), over the chunks the output's statistics count
// (n_chunks > 0).  measure: row_off[n_rows], chunk_bytes[n_chunks], *n_long += the long non-NULL cells; polr_launch_chunk_prefix
// over chunk_bytes gives chunk_heap_base.  write: heap_dev is where the bytes go, heap_addr the address the cells carry.
uint32_t polr_strout_block(const polr_out *o); // workgroup size of both, and of the fixed-width gather of polr_fromout.hip
void polr_launch_strout_measure(hipStream_t st, const polr_out *o, uint32_t slot, DevCol src, uint64_t *row_off,
                                uint64_t *chunk_bytes, unsigned long long *n_long);
void polr_launch_strout_write(hipStream_t st, const polr_out *o, uint32_t slot, DevCol src, const uint64_t *row_off,
                              const uint64_t *chunk_heap_base, uint4 *dst_cells, uint8_t *dst_valid, uint8_t *heap_dev,
                              uint64_t heap_addr);

// the joins and join orders of a pipeline request described to polr_pipeline_plan() (polr_capi.hip)
extern "C" void polr_pipeline_plan_joins(polr_ctx *ctx, const polr_join_desc *joins, uint32_t k, const int32_t *paths,
                                         uint32_t n_paths, PipePlanInput &in);

// shared between capi and mpx
int polr_plan_launch(polr_pipeline *p, bool materialize, uint64_t total_tuples, uint32_t *unit_size,
                     uint32_t *n_blocks_max);
uint32_t polr_resident_waves(polr_pipeline *p, bool materialize);
uint32_t polr_waves_per_block(polr_pipeline *p, bool materialize); // 0: does not fit at all
