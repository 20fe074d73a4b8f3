// duckdb-polr_amd/csrc/polr_pdict_plan.h -- the host rules of the dictionary of a VARCHAR PROBE column
// (polr_pipeline_encode_dictionary, polr_pipeline_fetch_dictionary[_codes]; include/polr_hip.h), as plain host code beside
// polr_dict_plan.h, whose sort layout, tile sizes and fetch rules hold here word for word.  No HIP in here: polr_dict.hip
// describes the request, asks the plan, and allocates and launches what the plan says; a stand-alone host program drives
// the header alone (tests/pdictplan/pdict_plan_main.cpp).
//
// Every refusal, in this order, each with its message:
//
//   polr_pdict_plan_encode       polr_pipeline_encode_dictionary
//     1. a flag other than POLR_DICT_SORTED, POLR_DICT_NULL_INVALID, POLR_DICT_SELECTED   POLR_E_INVALID
//     2. no such probe column                                                 POLR_E_INVALID
//     3. not a column of 16-byte string cells                                 POLR_E_INVALID
//     4. the column is encoded already (names its code column)                POLR_E_INVALID
//     5. the column is itself a code column                                   POLR_E_INVALID
//     6. the string table's slots exceed the 32-bit slot space                POLR_E_UNSUPPORTED
//
//   polr_pdict_plan_outcome      ... once the device has answered: the rules of polr_dict_plan_outcome in their order
//     1. a HIP error                                                          POLR_E_HIP
//     2. strings longer than 12 bytes, but the column's heap never came       POLR_E_INVALID
//     3. the string table filled up (capacity >= 2 x rows: cannot happen)     POLR_E_HIP
//
//   polr_pdict_plan_fetch        the fetch calls: polr_dict_plan_fetch, with the pipeline's wording of rule 1
//
// Two modes.  Over all rows every row is inserted.  With POLR_DICT_SELECTED and a selection in force only the positions
// of the selection are (n_insert = its length, duplicates included), and what need not be indexed by table row is sized by
// that count: polr_pdict_layout says which array is which.
#pragma once

#include "polr_dict_plan.h"

struct PolrPDictRequest {
	uint32_t flags, probe_col;
	uint32_t n_probe_cols;
	uint32_t width;       // of the probe column (read where probe_col < n_probe_cols)
	bool encoded;         // a dictionary of this column exists ...
	uint32_t encoded_as;  // ... and this is its code column
	bool is_code_col;     // the column is the code column of a dictionary
	uint64_t n_rows;      // rows of the probe table
	bool has_selection;   // a selection is in force ...
	uint64_t n_selected;  // ... of this many positions
};
struct PolrPDictPlan : PolrDictPlan {
	bool selected;     // the insert goes through the selection (the flag AND a selection in force)
	bool own_valid;    // selected && null_invalid: the code column gets `valid AND selected`, whatever the source has
	uint64_t n_insert; // positions inserted: the selection's length, or the table's rows
};

#define POLR_PDP_REFUSE(code_, ...)                                                                                    \
	do {                                                                                                               \
		snprintf(pl->err, sizeof(pl->err), __VA_ARGS__);                                                               \
		return (code_);                                                                                                \
	} while (0)

static inline int polr_pdict_plan_encode(const PolrPDictRequest &rq, PolrPDictPlan *pl) {
	*pl = PolrPDictPlan();
	if (rq.flags & ~(POLR_DICT_SORTED | POLR_DICT_NULL_INVALID | POLR_DICT_SELECTED)) {
		POLR_PDP_REFUSE(POLR_E_INVALID,
		                "dictionary flags 0x%x: only POLR_DICT_SORTED, POLR_DICT_NULL_INVALID and POLR_DICT_SELECTED are defined", rq.flags);
	}
	pl->sorted = (rq.flags & POLR_DICT_SORTED) != 0;
	pl->null_invalid = (rq.flags & POLR_DICT_NULL_INVALID) != 0;
	pl->selected = (rq.flags & POLR_DICT_SELECTED) != 0 && rq.has_selection;
	pl->own_valid = pl->selected && pl->null_invalid;
	pl->n_insert = pl->selected ? rq.n_selected : rq.n_rows;
	if (rq.probe_col >= rq.n_probe_cols) {
		POLR_PDP_REFUSE(POLR_E_INVALID, "probe column %u of %u", rq.probe_col, rq.n_probe_cols);
	}
	if (rq.width != 16) {
		POLR_PDP_REFUSE(POLR_E_INVALID, "a dictionary is made of a column of 16-byte string cells (this one: %u bytes)", rq.width);
	}
	if (rq.encoded) {
		POLR_PDP_REFUSE(POLR_E_INVALID, "probe column %u is encoded already (code column %u)", rq.probe_col, rq.encoded_as);
	}
	if (rq.is_code_col) {
		POLR_PDP_REFUSE(POLR_E_INVALID, "probe column %u is a code column: codes are not encoded again", rq.probe_col);
	}
	PolrCapacityPlan slots; // the string table: a slot space of its own, the build side's capacity rule
	if (polr_build_capacity(pl->n_insert, slots)) {
		POLR_PDP_REFUSE(POLR_E_UNSUPPORTED, "a dictionary over %llu %s rows exceeds the 32-bit slot space", (unsigned long long)pl->n_insert,
		                pl->selected ? "selected" : "probe");
	}
	pl->capacity = slots.capacity;
	return POLR_OK;
}

// hip_error: the text of the HIP error of the read-back, or NULL; n_long: the heap guard's count; full: the table's flag
static inline int polr_pdict_plan_outcome(const char *hip_error, unsigned long long n_long, bool full, uint32_t probe_col,
                                          PolrPDictPlan *pl) {
	if (int rc = polr_dict_plan_outcome(hip_error, 0, false, probe_col, pl)) {
		return rc;
	}
	if (n_long) {
		POLR_PDP_REFUSE(POLR_E_INVALID,
		                "probe column %u: %llu rows hold strings longer than 12 bytes, but the column's heap was never put on the device "
		                "(polr_pipeline_set_probe_heaps)",
		                probe_col, n_long);
	}
	return polr_dict_plan_outcome(nullptr, 0, full, probe_col, pl);
}

static inline int polr_pdict_plan_fetch(bool found, uint32_t code_col, uint32_t n_codes, const uint32_t *codes, uint64_t n,
                                        PolrPDictPlan *pl) {
	if (!found) {
		// (also a pipeline made by polr_pipeline_from_output of an output that carried a code column: the strings stay with
		// the pipeline that encoded)
		POLR_PDP_REFUSE(POLR_E_INVALID, "probe column %u is not a code column whose dictionary this pipeline holds", code_col);
	}
	return polr_dict_plan_fetch(true, code_col, n_codes, codes, n, pl);
}

// The encoder's single scratch allocation in either mode, in the order and rounding of polr_dict_layout:
//   per slot of the string table (capacity follows n_insert)   rep, hash, state, first_row, code
//   per TABLE ROW                                              slot_of_row (the rank and assign steps run over the table's
//                                                              rows: a row outside the selection holds "no slot"),
//                                                              block_sums (a word per POLR_DICT_BLOCK * POLR_DICT_ITEMS rows)
//   per INSERTED POSITION                                      row_of_code (there are no more codes than positions)
// n_insert == n_rows (every row is inserted): what polr_dict_layout(capacity, n_rows) returns, field for field.
static inline void polr_pdict_layout(uint64_t capacity, uint64_t n_rows, uint64_t n_insert, PolrDictLayout *lo) {
	polr_dict_layout(capacity, n_rows, lo); // (the table's arrays, slot_of_row and n_blocks are right already)
	const auto r16 = [](uint64_t bytes) { return (bytes + 15) & ~(uint64_t)15; };
	lo->block_sums = lo->row_of_code + r16(n_insert * 4);
	lo->scalars = lo->block_sums + r16((uint64_t)lo->n_blocks * 4);
	lo->n_long = lo->scalars + 32;
	lo->total = lo->scalars + 64;
}

#undef POLR_PDP_REFUSE
