// duckdb-polr_amd/csrc/polr_pipesrc_plan.h -- a polr_pipeline_from_output request checked and laid out, as plain host code.
// No HIP in here: polr_pipesrc.hip resolves the column references against the output's pipeline (polr_out_col), describes
// the joins as polr_pipeline_create does (PipePlanInput), hands both over with the output's counts, and allocates and
// launches what the plan says; a stand-alone host program drives the header alone (tests/pipesrc/pipesrc_plan_main.cpp).
//
// The plan composes the two plans that exist: the column layout of polr_ht_from_output (polr_fromout_plan.h) and the
// checks of polr_pipeline_create (polr_pipeline_plan.h).  It holds
//   * every refusal of the contract (include/polr_hip.h) in ITS ORDER, each with its message:
//       1. POLR_E_INVALID      the output, out, cols, joins or paths is NULL (in this order)
//       2. POLR_E_INVALID      n_cols == 0
//       3. POLR_E_UNSUPPORTED  more than POLR_PIPESRC_MAX_COLS columns
//       4. POLR_E_INVALID      the output has a fused GROUP BY sink
//       5. POLR_E_INVALID      a column reference out of range, the first one in the order of cols[]
//          (POLR_E_UNSUPPORTED a source cell that is not 1, 2, 4, 8 or 16 bytes wide)
//       6. POLR_E_UNSUPPORTED  an output of 2^32 - 16 rows or more
//       7. every refusal of polr_pipeline_plan() over the gathered columns as probe columns, with its own code and text
//     polr_pipesrc_check() is 1 to 4, what needs no column shape (it runs before the references are resolved);
//     polr_pipesrc_plan() is all of them;
//   * the probe columns of the new pipeline (in.probe_cols: width and signedness of the sources) and in.n_probe_rows;
//   * lay: the layout of polr_fromout_plan.h over all columns -- fixed[] by slot with the slot groups, strings[] with their
//     guards, the offsets of cells and validity arrays inside the single allocation, the descriptors behind them, and the
//     scratch of the string passes;
//   * pipe: the answer of polr_pipeline_plan().
#pragma once

#include "polr_fromout_plan.h"
#include "polr_pipeline_plan.h"

#define POLR_PIPESRC_MAX_COLS 66u       // the descriptor array the gather kernel reads through scalar loads was sized for 66
#define POLR_PIPESRC_MAX_ROWS 0xFFFFFFF0ull // probe row ids are 32-bit (the bound of polr_pipeline_create)

struct PolrPipesrcRequest {
	bool has_out, has_result, has_cols, has_joins, has_paths; // the pointers of the call that are not NULL
	bool fused;                                               // the output has a fused GROUP BY sink
	uint32_t n_cols;
	uint64_t n_rows, n_chunks; // of the output (polr_out_stats); polr_pipesrc_check does not read them
};

struct PolrPipesrcPlan {
	int code;
	char err[512];
	PolrFromoutPlan lay;
	PipePlan pipe;
};

#define POLR_PS_REFUSE(code_, ...)                                                                                     \
	do {                                                                                                               \
		snprintf(pl.err, sizeof(pl.err), __VA_ARGS__);                                                                 \
		return pl.code = (code_);                                                                                      \
	} while (0)

// refusals 1 to 4 -> POLR_OK, or POLR_E_* with pl.err set
static inline int polr_pipesrc_check(const PolrPipesrcRequest &rq, PolrPipesrcPlan &pl) {
	pl.err[0] = 0;
	pl.code = POLR_OK;
	if (!rq.has_out || !rq.has_result || !rq.has_cols || !rq.has_joins || !rq.has_paths) {
		POLR_PS_REFUSE(POLR_E_INVALID, "polr_pipeline_from_output: %s is NULL",
		               !rq.has_out      ? "the output"
		               : !rq.has_result ? "out"
		               : !rq.has_cols   ? "cols"
		               : !rq.has_joins  ? "joins"
		                                : "paths");
	}
	if (rq.n_cols == 0) {
		POLR_PS_REFUSE(POLR_E_INVALID, "polr_pipeline_from_output: no columns (a pipeline's source carries at least one)");
	}
	if (rq.n_cols > POLR_PIPESRC_MAX_COLS) {
		POLR_PS_REFUSE(POLR_E_UNSUPPORTED, "%u columns (at most %u)", rq.n_cols, POLR_PIPESRC_MAX_COLS);
	}
	if (rq.fused) {
		POLR_PS_REFUSE(POLR_E_INVALID, "the output has a fused GROUP BY sink: it holds group cells, no row ids to materialise");
	}
	return POLR_OK;
}

// cols[rq.n_cols]: the references as resolved; in: k, n_paths, joins, paths, device and flat_wave_bytes as
// polr_pipeline_create fills them -- probe_cols and n_probe_rows are written here -> POLR_OK, or POLR_E_* with pl.err set
static inline int polr_pipesrc_plan(const PolrPipesrcRequest &rq, const PolrFromoutColumn *cols, PipePlanInput &in,
                                    PolrPipesrcPlan &pl) {
	polr_fromout_clear(pl.lay);
	pl.lay.err[0] = 0;
	pl.pipe = PipePlan();
	if (polr_pipesrc_check(rq, pl)) {
		return pl.code;
	}
	for (uint32_t c = 0; c < rq.n_cols; c++) {
		if (!cols[c].resolved) {
			POLR_PS_REFUSE(POLR_E_INVALID, "column %u: no such column in the output's pipeline", c);
		}
		if (!polr_build_cell_width_ok(cols[c].width)) {
			POLR_PS_REFUSE(POLR_E_UNSUPPORTED, "column %u: cells of %u bytes", c, cols[c].width);
		}
	}
	if (rq.n_rows >= POLR_PIPESRC_MAX_ROWS) {
		POLR_PS_REFUSE(POLR_E_UNSUPPORTED, "output of %llu rows exceeds the 32-bit row-id space of a pipeline's source",
		               (unsigned long long)rq.n_rows);
	}
	in.probe_cols.clear();
	for (uint32_t c = 0; c < rq.n_cols; c++) {
		in.probe_cols.push_back(PipeCol {cols[c].width, cols[c].flags & POLR_COL_SIGNED});
	}
	in.n_probe_rows = rq.n_rows;
	if (polr_pipeline_plan(in, pl.pipe)) {
		POLR_PS_REFUSE(pl.pipe.code, "%s", pl.pipe.msg);
	}
	if (const int rc = polr_fromout_layout(rq.n_rows, rq.n_chunks, cols, rq.n_cols, pl.lay)) {
		POLR_PS_REFUSE(rc, "%s", pl.lay.err); // (cannot happen: slots are 0 .. POLR_MAX_JOINS)
	}
	return POLR_OK;
}
