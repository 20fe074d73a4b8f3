// duckdb-polr_amd/csrc/polr_pipesrc.hip -- polr_pipeline_from_output: the rows one pipeline emits as the SOURCE of the next,
// gathered on the device (a query of more than POLR_MAX_JOINS joins runs as several pipelines; this is the probe-side
// hand-over between two of them).  Probe row r of the new pipeline is output row r, chunk-major as polr_out_fetch_ids
// numbers them.  Contract: include/polr_hip.h; the request checked and laid out: polr_pipesrc_plan.h.
//
// The device work is that of polr_ht_from_output and is shared with it (polr_fromout_gather.h, the kernels in
// polr_fromout.hip and polr_strout.hip): ONE launch gathers every fixed-width column -- a workgroup per output chunk and
// slot group reads the row ids of its slot once and serves every column of that slot --, VARCHAR columns go through the
// measure and write passes, chunk bases come from the prefix over the chunks' fill counts.  Nothing here launches a kernel
// of its own.  Algorithmic bytes per output row: 4 read per distinct slot; w + 1 read and w + 1 written per column of w
// bytes; a VARCHAR column reads its cells twice (measure, write) and moves every long string's bytes once.
//
// Order: every refusal is decided on the host before anything but the output's statistics is enqueued; with a VARCHAR
// column the measuring passes run next and the heap-never-came guard is decided from what they read back; only then are
// the cells (one allocation for all cells, all validity arrays and the gather's descriptors: polr_pipeline::col_mem) and
// the heaps allocated and written.  The pipeline itself is then made by polr_pipeline_create over those arrays as
// POLR_COL_DEVICE columns -- the plan has accepted it already -- and takes the allocation and the heaps over.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <vector>

#include "polr_fromout_gather.h"
#include "polr_pipesrc_plan.h"

extern "C" int polr_pipeline_from_output(polr_out *o, void *stream, const polr_out_col_ref *cols, uint32_t n_cols,
                                         const polr_join_desc *joins, uint32_t k, const int32_t *paths, uint32_t n_paths,
                                         polr_pipeline **out) {
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
	PolrPipesrcRequest rq = {};
	rq.has_out = true;
	rq.has_result = out != nullptr;
	rq.has_cols = cols != nullptr;
	rq.has_joins = joins != nullptr;
	rq.has_paths = paths != nullptr;
	rq.fused = out_has_fused_sink(o);
	rq.n_cols = n_cols;
	auto plan_holder = std::make_unique<PolrPipesrcPlan>();
	PolrPipesrcPlan &plan = *plan_holder;
	if (polr_pipesrc_check(rq, plan)) {
		POLR_FAIL(ctx, plan.code, "%s", plan.err);
	}
	std::vector<OutCol> src(n_cols);
	std::vector<PolrFromoutColumn> shapes(n_cols);
	for (uint32_t c = 0; c < n_cols; c++) {
		POLR_TRY(polr_out_col(p, cols[c].src_join, cols[c].src_col, &src[c], "column", c));
		shapes[c] = polr_fromout_shape(src[c]);
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	POLR_TRY(out_ensure_stats(o, stream));
	const uint64_t n = o->n_rows; // (0 also for an output no materialising run has filled)
	const uint32_t nc = n ? o->n_chunks : 0;
	rq.n_rows = n;
	rq.n_chunks = nc;
	PipePlanInput in;
	polr_pipeline_plan_joins(ctx, joins, k, paths, n_paths, in);
	if (polr_pipesrc_plan(rq, shapes.data(), in, plan)) {
		POLR_FAIL(ctx, plan.code, "%s", plan.err);
	}
	const PolrFromoutPlan &lay = plan.lay;
	// VARCHAR columns: measure all of them, read back once, decide the guard
	const size_t ns = lay.strings.size();
	FromoutStrings fs;
	POLR_TRY(polr_fromout_measure(o, st, lay, src.data(), n, nc, fs));
	for (size_t s = 0; s < ns; s++) {
		const uint64_t n_long = fs.h_tails[2 * s + 1];
		if (n_long && lay.strings[s].needs_heap_guard) {
			// (the library's own upload, never rebased onto a device heap: the pointers of its long cells are the host's)
			POLR_FAIL_HEAP_NEVER_CAME(ctx, "column", lay.strings[s].col, n_long);
		}
	}
	// everything the new pipeline's source owns, before the first kernel that writes into it
	DevBuf<uint8_t> col_mem;
	std::vector<DevBuf<uint8_t>> heaps;
	HIPCHK(ctx, col_mem.alloc(lay.table_bytes));
	heaps.reserve(ns);
	for (size_t s = 0; s < ns; s++) {
		DevBuf<uint8_t> heap;
		HIPCHK(ctx, heap.alloc(fs.h_tails[2 * s]));
		heaps.push_back(std::move(heap));
	}
	std::vector<PolrFromoutDesc> h_desc;
	POLR_TRY(polr_fromout_fill(o, st, lay, src.data(), n, nc, fs, col_mem.get(), heaps, h_desc));
	HIPCHK(ctx, hipStreamSynchronize(st)); // (the columns are complete; the staged descriptors and the scratch are locals)
	// an ordinary pipeline over the gathered arrays
	std::vector<polr_col> pc(n_cols);
	for (uint32_t c = 0; c < n_cols; c++) {
		pc[c].data = col_mem.get() + lay.data_off[c];
		pc[c].valid = col_mem.get() + lay.valid_off[c];
		pc[c].width = shapes[c].width;
		pc[c].flags = shapes[c].flags | POLR_COL_DEVICE;
	}
	polr_pipeline *np = nullptr;
	POLR_TRY(polr_pipeline_create(ctx, pc.data(), n_cols, n, joins, k, paths, n_paths, &np));
	np->col_mem = std::move(col_mem);
	for (uint32_t c = 0; c < n_cols; c++) {
		np->probe_cols[c].lib_cells = true; // the library's own cells: not a caller's POLR_COL_DEVICE memory
	}
	for (size_t s = 0; s < ns; s++) {
		np->heaps.push_back(std::move(heaps[s]));
		np->probe_cols[lay.strings[s].col].strings_rebased = true;
	}
	*out = np;
	return POLR_OK;
}
