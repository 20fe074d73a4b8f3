// duckdb-polr_amd/csrc/polr_fromout_gather.h -- the columns of a pipeline's output gathered into one allocation: the device
// part that polr_ht_from_output (polr_fromout.hip, where it lives) and polr_pipeline_from_output (polr_pipesrc.hip) share.
// Both lay their columns out with polr_fromout_layout (polr_fromout_plan.h), call polr_fromout_measure, decide the
// heap-never-came guard from what it read back, allocate what the new handle owns, and call polr_fromout_fill.
#pragma once

#include <vector>

#include "polr_fromout_plan.h"
#include "polr_internal.h"

// a column reference as polr_out_col resolved it, in the plan's words
PolrFromoutColumn polr_fromout_shape(const OutCol &c);

// the string passes between measuring and writing: one scratch allocation and what was read back
struct FromoutStrings {
	DevBuf<uint64_t> scratch; // row offsets, chunk words, tails (per VARCHAR column: the heap bytes, the long cells)
	uint64_t *row_off = nullptr, *chunk_words = nullptr, *tails = nullptr;
	std::vector<uint64_t> h_tails; // [2 * strings]: h_tails[2 * s] the heap bytes of plan.strings[s], [2 * s + 1] its long non-NULL cells
};

// Measures every VARCHAR column of the plan over the n rows in nc chunks of `o` and reads the totals back: ONE
// synchronisation of `st`, none without such a column or without rows.  src[c]: column c as polr_out_col resolved it.
int polr_fromout_measure(polr_out *o, hipStream_t st, const PolrFromoutPlan &plan, const OutCol *src, uint64_t n, uint32_t nc,
                         FromoutStrings &fs);
// Enqueues everything that writes: the descriptors into mem + plan.desc_off, the gather of the fixed-width columns, the
// write pass of every VARCHAR column into heaps[s] (of h_tails[2 * s] bytes).  Column c's cells land at mem +
// plan.data_off[c], its validity array at mem + plan.valid_off[c].  h_desc is the staging of the descriptors: it must
// live until `st` has been synchronised, which is the caller's to do.
int polr_fromout_fill(polr_out *o, hipStream_t st, const PolrFromoutPlan &plan, const OutCol *src, uint64_t n, uint32_t nc,
                      const FromoutStrings &fs, uint8_t *mem, const std::vector<DevBuf<uint8_t>> &heaps,
                      std::vector<PolrFromoutDesc> &h_desc);
