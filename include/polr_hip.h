/*
 * include/polr_hip.h -- the drop-in boundary of the MI355X POLAR path.
 *
 * A thin C ABI (plain pointers and sizes, no C++/torch types) under the reference's operator
 * classes.  The reference (d-justen/duckdb-polr) has no FFI seam: PhysicalMultiplexer,
 * PhysicalHashJoin and PhysicalAdaptiveUnion are C++ classes linked into libduckdb, and the
 * boundary sits inside POLARPipelineExecutor::RunPath (src/parallel/polar_pipeline_executor.cpp:
 * 427-538).  Each entry point below names the reference code whose job it takes over; the
 * C++ host mirror in duckdb-polr_amd/host/ (same class names as the reference) is the only
 * intended caller, INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions: every call returns 0 on success or a negative POLR_E_* code; polr_last_error()
 * returns the text of the last failure of that context (thread-compatible: one context per host
 * thread, like one PipelineExecutor per thread in the reference).  The caller owns host buffers;
 * the library owns device buffers behind opaque handles.  `stream` is a hipStream_t passed as
 * void* (NULL = the context's own stream).  There is NO CPU fallback: without a visible gfx950
 * device polr_ctx_create fails with POLR_E_NO_DEVICE.
 */
#ifndef POLR_HIP_H
#define POLR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POLR_ABI_VERSION 1

#define POLR_MAX_JOINS 8   /* consecutive INNER hash joins multiplexed in one pipeline */
#define POLR_MAX_PATHS 32  /* >= max_join_orders used by the reference's experiments (24) */
#define POLR_MAX_KEYS 4    /* equality conditions per join.  Two columns of <= 32 bits, or one of <= 64, are compared as
                            * they are; any other combination (3 or 4 keys, a wide column in a composite) is packed
                            * EXACTLY into 64 bits from the build side's per-column [min, max] (sum of the columns' range
                            * bits <= 64, else POLR_E_UNSUPPORTED): never a hash, so no verification pass */

enum {
	POLR_OK = 0,
	POLR_E_NO_DEVICE = -1,
	POLR_E_INVALID = -2,     /* bad argument / shape mismatch (checked on the host before any launch) */
	POLR_E_UNSUPPORTED = -3, /* type or plan shape outside the path (fails loudly, never falls back) */
	POLR_E_HIP = -4,         /* a HIP runtime call failed; text in polr_last_error */
	POLR_E_DUPLICATE = -5,   /* perfect-hash build saw a duplicate key: caller keeps the chained table,
	                            like perfect_hash_join_executor.cpp:112-114 */
	POLR_E_OVERFLOW = -6,    /* output buffer too small; counters are still exact */
	POLR_E_RANGE = -7        /* an aggregate argument `left OP right` lies outside its result type for some output row: the
	                            reference's OutOfRangeException ("Overflow in multiplication of ..."); no result is written */
};

/* MultiplexerRouting (src/include/duckdb/main/config.hpp:41-50), same order */
enum {
	POLR_ROUTE_ALTERNATE = 0,
	POLR_ROUTE_ADAPTIVE_REINIT = 1,
	POLR_ROUTE_DYNAMIC = 2,
	POLR_ROUTE_INIT_ONCE = 3,
	POLR_ROUTE_OPPORTUNISTIC = 4,
	POLR_ROUTE_DEFAULT_PATH = 5,
	POLR_ROUTE_BACKPRESSURE = 6,
	POLR_ROUTE_EXPONENTIAL_BACKOFF = 7
};

typedef struct polr_ctx polr_ctx;           /* one device + one stream + error text */
typedef struct polr_ht polr_ht;             /* a finalized build side resident in HBM */
typedef struct polr_pipeline polr_pipeline; /* probe columns + joins + join orders (POLARConfig) */
typedef struct polr_out polr_out;           /* chunked output of a run (DataChunk stream) */
typedef struct polr_mpx polr_mpx;           /* device-resident multiplexer state + router */

/* A flat column (FLAT vector after ToUnifiedFormat, src/include/duckdb/common/types/vector.hpp:22-27).
 * valid: NULL = all valid, else one byte per row (1 = valid).  width in bytes: 1, 2, 4, 8 or 16
 * (16 = string_t copied as an opaque cell, row_gather.cpp:47-86). */
#define POLR_COL_SIGNED 1u
#define POLR_COL_DEVICE 2u /* data/valid are device pointers (e.g. torch tensors) */
typedef struct polr_col {
	const void *data;
	const uint8_t *valid;
	uint32_t width;
	uint32_t flags;
} polr_col;

/* ---------------------------------------------------------------------------------------------
 * Context
 * ------------------------------------------------------------------------------------------- */
int polr_abi_version(void);
int polr_ctx_create(int device_id, polr_ctx **out);
void polr_ctx_destroy(polr_ctx *ctx);
const char *polr_last_error(const polr_ctx *ctx);
int polr_ctx_sync(polr_ctx *ctx, void *stream);
/* The context's own stream (what `stream == NULL` means for every call except the multiplexer runs, which default to a
 * stream of the first multiplexer): pass it to polr_mpx_run_resident* to put a run in line with polr_out_reset before
 * it and polr_out_aggregate* behind it -- a pass with its sink is then one ordered sequence, no host synchronisation. */
int polr_ctx_get_stream(polr_ctx *ctx, void **stream);
/* Tuning of the pool launch (polr_mpx_run_resident*): how a context's runs cut rounds into units and how its probe
 * waves poll.  A field left 0 keeps the library's default; NULL restores every default.  Results never depend on any
 * of these (only speed does), except watchdog_us, which bounds how long a router waits for its probe waves before the
 * run is given up with POLR_E_HIP.  Takes effect with the next run of the context. */
typedef struct polr_pool_tuning {
	uint32_t device_share; /* size every run's grid for 1/device_share of the device (1..16); 0: as the run's flags say */
	uint32_t units_x;      /* a big round is cut into about units_x x probe waves / routing executors units (1..4; default 4) */
	uint32_t hi_unit;      /* tuples per unit of a small round: 64..1024, a multiple of 64 (default: 1024 flat; generic 64,
	                          with more than 64 executors 256) */
	uint32_t hi_lottery;   /* power of two: wave w of a ring tries for hi ticket t only if w % lottery == t % lottery */
	uint32_t hi_tuples_p1; /* 1 + the size up to which a round counts as small (default 4096); 0: default */
	uint32_t idle_sleep;   /* 16: an idle probe wave's back-off stays at s_sleep 16 (default 64) */
	uint32_t watchdog_us;  /* microseconds; default 4 000 000 */
	uint32_t share_after;  /* work sharing (pipelines with repeated build keys): a probe wave that has spent this many
	                          steps on ONE unit gives half of what it still has to do -- the rest of its source range,
	                          of a run of build rows, or of the tuples waiting between two joins -- to the pool, and
	                          again after as many steps (16..65535; default 32: measured 16 / 32 / 64 / 128 on the 113 JOB-shaped
	                          pipelines); 0xFFFFFFFF: never */
} polr_pool_tuning;
int polr_ctx_set_pool_tuning(polr_ctx *ctx, const polr_pool_tuning *tuning);
/* Diagnostic: bytes of device memory the library owns right now, over every context and handle of the process -- what
 * a leak test compares before and after (exact, where the device's free memory also moves with other tenants).  Not
 * counted: pinned host memory, streams, events, RCCL's own buffers. */
uint64_t polr_device_bytes_live(void);

/* ---------------------------------------------------------------------------------------------
 * Build sides.  Replaces what JoinHashTable::Finalize leaves in host memory
 * (src/execution/join_hashtable.cpp:324-377) with a device-native layout:
 *   - keys/payload de-serialised into SoA columns indexed by build row,
 *   - an open-addressing bucket array: 8-byte {key,row} slots for a unique 32-bit key, 16-byte
 *     {key64,start,count} slots + a row-id run array when the key repeats (bucket-contiguous
 *     instead of pointer-chained: the reference's chain order is not part of its contract,
 *     join_hashtable.cpp:284-303),
 *   - or the direct-address perfect table of perfect_hash_join_executor.cpp:20-122.
 * Build row ids reported anywhere in this API are the ordinals of the rows as uploaded.
 * ------------------------------------------------------------------------------------------- */

/* Upload the reference's row-format blob (RowLayout, src/common/types/row_layout.cpp:19-80;
 * JoinHashTable ctor join_hashtable.cpp:43-57): n_rows rows of row_width bytes, column i at
 * col_offset[i] (keys first, then payload), validity bits at the front of each row.  The
 * reference's own bucket array is not needed: the device re-buckets. */
int polr_ht_upload_rows(polr_ctx *ctx, const void *rows, uint64_t n_rows, uint32_t row_width,
                        const uint32_t *col_offset, const uint32_t *col_width, const uint32_t *col_flags,
                        uint32_t n_keys, uint32_t n_payload, polr_ht **out);
/* Same from columnar build data (DataChunks as sunk by PhysicalHashJoin::Sink,
 * physical_hash_join.cpp:217-286).  Rows with a NULL key are dropped (join_hashtable.cpp:170-192) unless the
 * column is POLR_KEY_NULL_EQUAL; row ids still refer to the rows as passed. */
int polr_ht_upload_columns(polr_ctx *ctx, const polr_col *keys, uint32_t n_keys, const polr_col *payload,
                           uint32_t n_payload, uint64_t n_rows, polr_ht **out);
/* Same from the OUTPUT of another pipeline, on the device: the pipeline whose sink is the build of a hash join
 * (PhysicalHashJoin::Sink of a child pipeline, physical_hash_join.cpp:217-286; the bushy plans of JOB).  `o` is an output a
 * materialising run has filled; keys[i] / payload[i] name columns of its pipeline as polr_agg_spec does.
 * The new table is un-finalized, exactly as polr_ht_upload_columns would return it, with ONE BUILD ROW PER OUTPUT ROW of `o`
 * in the order of polr_out_fetch_ids / polr_out_materialize (chunk-major): build row id r of the new table is output row r
 * of `o`, so a pipeline that later probes the new table reports ids that index polr_out_fetch_ids of `o`.
 * Columns: column i has the width and the POLR_COL_SIGNED flag of its source; every column gets a validity array gathered
 * from the source's (all rows valid when the source has none); the cell of a NULL row is zero and the source cell of a NULL
 * row is never read.  Keys: the shapes polr_ht_upload_columns takes -- 1..POLR_MAX_KEYS columns of 1, 2, 4 or 8 bytes (a
 * 16-byte key: POLR_E_UNSUPPORTED); at most 62 payload columns (what polr_ht_export carries).  The same source column may
 * be named more than once, also once as a key and once as payload.
 * Afterwards polr_ht_set_key_flags, the three polr_ht_finalize_* calls, polr_ht_encode_dictionary[_ex], polr_ht_get_info and
 * -- for a table without VARCHAR columns -- polr_ht_export / polr_ht_alloc_like work as on any uploaded table; rows with a
 * NULL key are dropped at finalize as always.
 * VARCHAR payload columns (width 16): the cells are normalised exactly as polr_out_materialize_strings normalises them
 * (inline strings zero-padded, NULL rows all-zero) and the long strings' bytes are copied into a packed heap THE NEW TABLE
 * OWNS, one per such column; the column counts as rebased, so a later polr_ht_set_payload_heaps on it is refused.  A source
 * column the library uploaded whose heap never came is POLR_E_INVALID once a long non-NULL cell is among the output rows
 * (decided by the measuring pass, before any pointer is followed).
 * Ownership: when the call returns the new table shares nothing with `o`, its pipeline, the source tables or a caller's
 * POLR_COL_DEVICE memory -- all of those may be destroyed; it holds a reference to the context as every handle does, and
 * polr_ht_info::device_bytes and polr_device_bytes_live() account for every byte of it.
 * Refusals -- nothing is enqueued beyond the output's own statistics, *out = NULL, polr_device_bytes_live() as before:
 *   POLR_E_INVALID      NULL o, out or keys; NULL payload with n_payload > 0; an output with a fused GROUP BY sink (it holds
 *                       group cells, no row ids); a column reference out of range
 *   POLR_E_UNSUPPORTED  n_keys outside 1..POLR_MAX_KEYS, a key wider than 8 bytes, more than 62 payload columns; an output
 *                       of 2^32 - 16 rows or more (the bound of polr_ht_upload_columns)
 * An output with no rows, or one no materialising run has filled, gives a valid table of 0 rows: it finalizes, and probing
 * it matches nothing.  The call returns when the table is complete (it needs the row count on the host, and with a VARCHAR
 * column the heap totals). */
typedef struct polr_out_col_ref {
	int32_t src_join; /* -1 = probe-table column, j >= 0 = payload column of join j (as polr_agg_spec) */
	uint32_t src_col;
} polr_out_col_ref;
int polr_ht_from_output(polr_out *o, void *stream, const polr_out_col_ref *keys, uint32_t n_keys,
                        const polr_out_col_ref *payload, uint32_t n_payload, polr_ht **out);
/* Filter the rows of an UN-FINALIZED table and compact it, on the device: the filtered dimension scan in front of
 * PhysicalHashJoin::Sink (physical_hash_join.cpp:217-286) -- the PhysicalFilter, or the TableFilterSet pushed into the scan,
 * that nearly every build pipeline of SSB and JOB carries (c_region = 'AMERICA', k.keyword LIKE '%sequel%').  Call it after
 * the upload and before polr_ht_encode_dictionary[_ex] and polr_ht_finalize_*: the perfect range, the hash capacity and the
 * dictionary codes are then those of the surviving rows.
 * Program: exactly a polr_pipeline_scan_filter_expr program (below) -- postfix nodes[] / values[] under SQL three-valued
 * logic, CMP incl. IS [NOT] NULL, IN, LIKE, NOT / AND / OR; a row is kept iff the root is TRUE; n_nodes == 0 keeps every
 * row.  nodes[i].col numbers the table's columns as polr_ht_upload_rows does, keys first, then payload: col < n_keys is key
 * column col, otherwise payload column col - n_keys.  The limits are those of the scan call (POLR_MAX_FILTER_*, 8 distinct
 * columns, no NUL in a pattern) and every refusal of that call's program check passes through with its message behind
 * "filter expression: ".  A CMP, IN or LIKE leaf on a NULL row is NULL and the row's cell is never read.
 * Tables: any un-finalized table -- from polr_ht_upload_columns (host or POLR_COL_DEVICE columns), polr_ht_upload_rows or
 * polr_ht_from_output.  POLR_E_INVALID, checked in this order before anything is enqueued: NULL ht; a finalized table (also
 * polr_pht_upload, polr_ht_alloc_like); a table with a dictionary-encoded column (filter first, then encode); a table
 * filtered before (once per table); then the program's refusals, `col` beyond the table's columns among them.  n_kept may
 * be NULL.
 * Result: the table holds exactly the kept rows, in ascending order of the rows as uploaded: build row r is now the r-th
 * kept row, and every build id reported later indexes polr_ht_fetch_filter_rows, which returns the uploaded row number of
 * every build row (dst_rows >= the kept count, else POLR_E_OVERFLOW; POLR_E_INVALID on a table that was never filtered).
 * Like the dictionary strings the row list stays with the table that was filtered: polr_ht_export / polr_ht_alloc_like /
 * polr_bcast_build do not carry it.  Widths, POLR_COL_SIGNED, key flags and the payload count are unchanged; a column has
 * a validity array afterwards iff it had one before; the cell of a kept NULL row is zero (its source is not read), a kept
 * valid cell is copied bit for bit.
 * VARCHAR columns: cells are copied as they are and keep pointing into the heap the table already owns (or, for
 * POLR_COL_DEVICE cells, into the caller's HBM).  polr_ht_set_payload_heaps may come before or after the call for a column no
 * leaf reads; afterwards it checks and rebases the kept cells only.  A column some CMP / IN / LIKE leaf reads needs its
 * heap first: a column the library uploaded whose heap never came and that holds a non-NULL cell longer than 12 bytes is
 * POLR_E_INVALID, from a pass over the length words before a kernel that follows a pointer is enqueued.
 * Ownership: after the call the table owns the cells and validity arrays of ALL its columns in ONE allocation (with the row
 * list); a caller's POLR_COL_DEVICE buffers are never written and no longer referenced -- except that the VARCHAR cells of
 * such a column still point into the caller's heap, which must outlive the table.  The buffers the table owned before are
 * freed before the call returns; polr_ht_info::device_bytes and polr_device_bytes_live() account for the new state.  A
 * refused or failed call leaves the table, its columns and the live byte count exactly as they were.
 * Stream: as polr_ht_encode_dictionary -- the call waits for the context's stream and returns when the table is complete
 * (it needs the kept count on the host once, between its counting and its compaction pass).
 * Not provided: filtering a finalized table; repacking the string heaps (the bytes of dropped rows stay); a second
 * polr_ht_filter on one table (thinning by other tables composes: polr_ht_semi_filter, below); shipping the row list through
 * polr_bcast_build; pipelines of zero joins. */
struct polr_filter_node; /* (defined with polr_pipeline_scan_filter_expr, below) */
struct polr_filter_value;
int polr_ht_filter(polr_ht *ht, void *stream, const struct polr_filter_node *nodes, uint32_t n_nodes,
                   const struct polr_filter_value *values, uint32_t n_values, uint64_t *n_kept);
int polr_ht_fetch_filter_rows(polr_ht *ht, void *stream, uint32_t *dst, uint64_t dst_rows);
/* Thin an UN-FINALIZED table by SEMI / ANTI joins against other, finalized tables and compact it, on the device: the SEMI /
 * ANTI / MARK hash joins inside a build subtree that ExtractInfoLinear walks through as predicates on the base table
 * (src/parallel/polar_enumeration_algo.cpp:192-205; ScanStructure::NextSemiJoin / NextAntiJoin,
 * src/execution/join_hashtable.cpp:589-627) -- a dimension restricted by k IN (SELECT ...), EXISTS or NOT EXISTS -- and the
 * semi-join reduction of a large build side by the keys of a small filtered table.  It is LIP for build sides: the index of
 * `by` is the filter, without false positives.
 * Match rule: a row MATCHES filter f iff its key, read from the columns cols[] of `ht`, would find at least one build row of
 * f.by if it were a probe tuple of a join on f.by.  So: a NULL in a key column never matches unless that key column of `by`
 * carries POLR_KEY_NULL_EQUAL (then it matches iff `by` kept a NULL key there); a value outside the range of a
 * POLR_KEY_BY_VALUE / packed column never matches; a key that repeats in `by` counts once; the all-ones 8-byte key is found
 * through the side entry a run hash table keeps for it.
 * Kept rows: flags == 0 (SEMI) keeps the matching rows; POLR_SEMI_ANTI keeps the rest -- rows whose key is NULL among them.
 * That is NOT EXISTS (NextSemiOrAntiJoin<false>: NULL keys never enter the match selection).  NOT IN over a NULL-free
 * subquery is polr_ht_filter(key IS NOT NULL) followed by an ANTI filter; the NULL propagation of a MARK join whose subquery
 * holds NULLs stays with the engine.
 * Several filters: a row is kept iff every filter keeps it (the device tests the smallest `by` first; the order changes the
 * work, never the survivors).  n_filters == 0 keeps every row but still compacts and sets the row list.
 * Columns: cols[] numbers the columns of `ht` as a polr_ht_filter program does, keys first, then payload; column cols[c]
 * is compared with key c of `by` under the rule of a join's keys: same width unless that key carries POLR_KEY_BY_VALUE,
 * integer widths only.  `by` may be any finalized table: a perfect table, a unique-key or a run hash table, its key in the
 * plain form (one key, or two of <= 32 bits) or the packed form (up to four keys, by value, NULL = NULL).  Nothing verifies
 * strings or wide composites here: a cols[] entry that names a 16-byte column is POLR_E_UNSUPPORTED, and a `by` keyed by a
 * hash of strings is compared ON THE HASH ALONE.
 * Composition: the call is allowed on a table polr_ht_filter or an earlier polr_ht_semi_filter has filtered;
 * polr_ht_fetch_filter_rows then returns the composed list -- the row numbers AS UPLOADED of the rows that are left.
 * polr_ht_filter after this call stays refused ("filtered already"): constant filters go first.
 * Everything else is as polr_ht_filter: the result is compacted in upload order into one allocation the table owns (a table
 * filtered before also keeps, unused, the 4-byte list of this pass); a caller's POLR_COL_DEVICE buffers are never written;
 * VARCHAR cells are copied as they are; a column has a validity array afterwards iff it had one; device_bytes and
 * polr_device_bytes_live() account for the new state; the call waits for the context's stream and returns when the table is
 * complete.  `by` is only read and may be destroyed after the call returns.
 * Refusals, checked in this order before anything is enqueued -- the table, its columns and the live byte count stay exactly
 * as they were: NULL ht; a finalized ht; a dictionary-encoded ht (POLR_E_INVALID); n_filters > POLR_MAX_SEMI_FILTERS
 * (POLR_E_UNSUPPORTED); NULL filters with n_filters > 0; then per filter, in order: NULL by; by not finalized; by == ht; by
 * on another device or context; unknown flag bits; n_cols != by's key count; and per key a cols[] entry beyond the table's
 * columns (all POLR_E_INVALID), a 16-byte column (POLR_E_UNSUPPORTED), the pairing rule.  n_kept may be NULL.
 * Not provided: non-equality or verifying conditions; MARK columns as output; filtering a finalized table; shipping the row
 * list through polr_bcast_build. */
#define POLR_SEMI_ANTI 1u /* keep the rows WITHOUT a match (NOT EXISTS); 0: keep the rows WITH one */
#define POLR_MAX_SEMI_FILTERS 4
typedef struct polr_semi_filter {
	const polr_ht *by;            /* a FINALIZED table on the same device */
	uint32_t n_cols;              /* == by's key count */
	uint32_t cols[POLR_MAX_KEYS]; /* columns of `ht`, numbered as polr_ht_filter numbers them: keys first, then payload */
	uint32_t flags;               /* 0 or POLR_SEMI_ANTI */
} polr_semi_filter;
int polr_ht_semi_filter(polr_ht *ht, void *stream, const polr_semi_filter *filters, uint32_t n_filters, uint64_t *n_kept);
/* Key semantics beyond "same type on both sides, NULL never matches": the reference multiplexes INNER hash joins whose
 * left side is CAST(column) (src/parallel/polar_config.cpp:75-82) and whose comparison is IS NOT DISTINCT FROM
 * (JoinHashTable::null_values_are_equal, src/execution/join_hashtable.cpp:35-36,170-192,642).  Per key column, BEFORE the
 * table is finalized:
 *   POLR_KEY_BY_VALUE    compare this column BY VALUE whatever integer type the probe side reads (an integer CAST on
 *                        either side of the condition): widths and signedness of the two sides may differ, a probe
 *                        value the build side does not hold never matches.  No cast copy of the probe column is made.
 *   POLR_KEY_NULL_EQUAL  IS NOT DISTINCT FROM: NULL = NULL on this column; build rows whose key is NULL there are kept.
 * A table with such a column is a hash table with its key in packed form (polr_ht_finalize_hash, _auto;
 * polr_ht_finalize_perfect refuses: the reference plans perfect hash joins for plain equalities only). */
#define POLR_KEY_BY_VALUE 1u
#define POLR_KEY_NULL_EQUAL 2u
int polr_ht_set_key_flags(polr_ht *ht, uint32_t key_col, uint32_t flags);
/* Finalize as a hash table (JoinHashTable::Finalize / InsertHashes, join_hashtable.cpp:305-377). */
int polr_ht_finalize_hash(polr_ht *ht, void *stream);
/* Finalize as a perfect hash table (BuildPerfectHashTable, perfect_hash_join_executor.cpp:20-122):
 * keys outside [min,max] are skipped; a duplicate inside the range returns POLR_E_DUPLICATE and
 * leaves the handle un-finalized so the caller can polr_ht_finalize_hash it instead. */
int polr_ht_finalize_perfect(polr_ht *ht, int64_t min_value, int64_t max_value, void *stream);
/* Let the device pick the index: a single integer key whose value range [min,max] (the build column's
 * statistics, as PerfectHashJoinStats carries them: build_min / build_max) is at most POLR_DENSE_FACTOR x
 * the build rows -- or at most 1 000 000 values, the reference planner's own bound (plan_comparison_join.cpp:118,125) --
 * becomes a perfect table (1 bit per key value: 3 M dense keys = 375 KB, L2-resident, where a
 * bucket table would cost one random 64-B HBM line per probe) -- the reference's own perfect-hash idea without
 * its 1 M-value cap (perfect_hash_join_executor.cpp:25-50), which was sized for CPU caches; anything else,
 * and a range with a duplicate key, becomes a hash table.  Match sets are identical either way; *kind_out
 * (may be NULL) tells which build-id convention applies (see polr_ht_get_info). */
#define POLR_DENSE_FACTOR 8
int polr_ht_finalize_auto(polr_ht *ht, int64_t min_value, int64_t max_value, void *stream, uint32_t *kind_out);
/* Column statistics on the device: what the reference's planner carries as NumericStatistics min / max into
 * PerfectHashJoinStats (build_min / build_max / probe_min / probe_max, plan_comparison_join.cpp:63-133) and into the group
 * domains of PhysicalPerfectHashAggregate, for columns that never were on the host -- a table made by polr_ht_from_output or
 * thinned by polr_ht_filter / polr_ht_semi_filter, a pipeline made by polr_pipeline_from_output.  One call is one pass over
 * the named columns; min_value / max_value are what polr_ht_finalize_perfect / polr_ht_finalize_auto take, and min_value and
 * max_value - min_value + 1 are the min_value / n_values of a polr_group_key.
 * Values: a POLR_COL_SIGNED column is compared and returned sign-extended, any other column zero-extended; an unsigned
 * 8-byte column is compared as unsigned and returned as its bit pattern (the convention of polr_ht_finalize_auto: the two
 * numbers can be handed on unchanged).  With n_valid == 0, min_value and max_value are both 0: look at n_valid.
 * NULL rows: a row whose validity byte is 0 takes no part, whatever its cell holds.
 * VARCHAR columns (width 16): min_value / max_value are the minimum and maximum LENGTH in bytes of the non-NULL strings,
 * n_long counts those longer than 12 bytes and long_bytes sums their lengths (what a packed heap of them takes).  Only the
 * length word of a cell is read and no pointer is followed: the call needs no heap and never refuses for one that never came.
 * polr_ht_column_stats: cols[] numbers the table's columns as a polr_ht_filter program does, keys first, then payload
 * (dictionary code columns are ordinary 4-byte payload columns); the same column may be named more than once.  Any
 * UN-FINALIZED table, whatever its route (polr_ht_upload_columns with host or POLR_COL_DEVICE columns, polr_ht_upload_rows,
 * polr_ht_from_output), also after polr_ht_filter, polr_ht_semi_filter and polr_ht_encode_dictionary*: the statistics
 * describe the rows the table holds now.
 * polr_pipeline_column_stats: cols[] are probe columns, over all n_probe_rows; with POLR_STATS_SELECTED only over the rows of
 * the selection in force (polr_pipeline_set_selection or one of the scan-filter calls; with none in force: all rows).  Any
 * pipeline, from polr_pipeline_create (host or device columns) or polr_pipeline_from_output.
 * Zero rows -- a table or pipeline of none, an empty selection --: n_rows = n_valid = 0 for every column, nothing is
 * launched.
 * Refusals, checked in this order -- nothing is enqueued, stats is untouched, the live bytes are as before: a NULL handle,
 * cols or stats; n_cols == 0 (POLR_E_INVALID); n_cols > POLR_MAX_STATS_COLS (POLR_E_UNSUPPORTED); a finalized table, also one
 * from polr_pht_upload or polr_ht_alloc_like / unknown flag bits of the pipeline call; a cols[] entry beyond the columns, the
 * first one in order (POLR_E_INVALID).
 * The calls wait for the context's stream and return when the numbers are on the host (as polr_ht_encode_dictionary);
 * the scratch -- one partial record per workgroup -- is allocated and freed inside the call: polr_device_bytes_live() is
 * afterwards what it was; a caller's POLR_COL_DEVICE memory is only read.
 * polr_ht_finalize_auto_stats: polr_ht_finalize_auto with the statistics taken here.  One plain key (n_keys == 1, no key
 * flags): the statistics of key column 0, NULL keys apart -- the rows that enter the table --; with at least one non-NULL key
 * exactly polr_ht_finalize_auto(ht, min_value, max_value, stream, kind_out): same index kind, same build-id convention, same
 * polr_ht_get_info, same fallback to a hash table on a duplicate; with none polr_ht_finalize_hash.  Several keys or a flagged
 * key: polr_ht_finalize_hash as in polr_ht_finalize_auto, and no statistics pass unless key_stats is given.  key_stats may be
 * NULL; when given it is filled for key column 0 in every case.  Refusals: those of polr_ht_finalize_auto.
 * Not provided: statistics of a finalized table or of output rows (polr_out_aggregate MIN / MAX covers those); distinct
 * counts or uniqueness. */
#define POLR_MAX_STATS_COLS 16
#define POLR_STATS_SELECTED 1u   /* pipeline call: only the rows of the selection in force */
typedef struct polr_col_stats {
	int64_t  min_value, max_value; /* integer column: over the non-NULL rows, in the column's own order */
	uint64_t n_rows;               /* rows looked at */
	uint64_t n_valid;              /* of them non-NULL */
	uint64_t n_long;               /* VARCHAR: non-NULL strings longer than 12 bytes (0 for integer columns) */
	uint64_t long_bytes;           /* VARCHAR: sum of their lengths (what a packed heap of them takes) */
	uint32_t width, flags;         /* of the column: 1/2/4/8/16, POLR_COL_SIGNED */
} polr_col_stats;
int polr_ht_column_stats(polr_ht *ht, void *stream, const uint32_t *cols, uint32_t n_cols, polr_col_stats *stats);
int polr_pipeline_column_stats(polr_pipeline *p, void *stream, const uint32_t *cols, uint32_t n_cols, uint32_t flags,
                               polr_col_stats *stats);
int polr_ht_finalize_auto_stats(polr_ht *ht, void *stream, uint32_t *kind_out, polr_col_stats *key_stats);
/* Diagnostic, launches nothing: what a statistics call plans for ONE column of n_rows rows and `width` bytes whose cells
 * start at a 16-byte boundary and are not read through a selection (POLR_E_INVALID: NULL info or a width that is none of
 * 1/2/4/8/16). */
typedef struct polr_col_stats_plan {
	uint32_t cells_per_load;  /* cells one 16-byte load of a lane brings */
	uint32_t loads_in_flight; /* independent loads a lane issues together */
	uint32_t tile_rows;       /* rows of a workgroup tile */
	uint32_t n_workgroups;    /* workgroups launched (0: no rows, nothing launched) */
	uint64_t stride_rows;     /* rows the grid covers before a workgroup takes its second tile */
	uint64_t scratch_bytes;   /* the partial records */
} polr_col_stats_plan;
int polr_col_stats_plan_info(uint64_t n_rows, uint32_t width, polr_col_stats_plan *info);
/* Upload a perfect table the reference already built (PerfectHashJoinExecutor members
 * perfect_hash_table / bitmap_build_idx, perfect_hash_join_executor.hpp): bitmap has range+1
 * bools, each payload column has range+1 cells. */
int polr_pht_upload(polr_ctx *ctx, uint32_t key_width, uint32_t key_flags, int64_t min_value, int64_t max_value,
                    const uint8_t *bitmap, const polr_col *payload, uint32_t n_payload, polr_ht **out);
void polr_ht_destroy(polr_ht *ht);

typedef struct polr_ht_info {
	uint32_t kind;      /* 0 = not finalized, 1 = perfect, 2 = hash {key,row} slots, 3 = hash {key,start,count} slots */
	uint32_t n_keys;
	uint64_t n_rows;    /* rows kept (NULL keys dropped) */
	uint64_t capacity;  /* hash slots, or range+1 */
	uint64_t max_run;   /* longest duplicate run */
	uint64_t device_bytes;
	uint32_t is_dense;  /* perfect: every slot of the range filled and no NULL build key */
	uint32_t has_null;
} polr_ht_info;
int polr_ht_get_info(const polr_ht *ht, polr_ht_info *info);
/* Broadcast support (RCCL, one exchange per build side): device pointers + byte sizes of the
 * buffers that make up the finalized table, so the caller (torch.distributed, backend "nccl")
 * can broadcast them in place.  The receiving rank first creates a same-shaped empty table with
 * polr_ht_alloc_like from the metadata blob. */
int polr_ht_export(const polr_ht *ht, void *meta, uint64_t *meta_bytes, void **dev_ptrs, uint64_t *dev_bytes,
                   uint32_t *n_buffers);
int polr_ht_alloc_like(polr_ctx *ctx, const void *meta, uint64_t meta_bytes, polr_ht **out);

/* ---- multi-GPU: the one exchange step of the path ----------------------------------
 * One POLAR pipeline per GPU (own multiplexer state, own probe partition) is the counterpart of one PipelineExecutor
 * per worker thread (src/parallel/pipeline.cpp:145-174); the only data every pipeline needs and only one has is the
 * finalized build side (JoinHashTable::Finalize, src/execution/join_hashtable.cpp:324-377).  polr_bcast_build ships
 * it from the rank that built it to all others with ncclBroadcast over xGMI (RCCL, loaded on first use): metadata,
 * then every device buffer in place.  Collective: every rank calls it, in the same order.  root: *ht is the table to
 * send; other ranks: *ht receives a new table (caller destroys it).  The 128-byte id comes from
 * polr_comm_get_unique_id on one rank and reaches the others out of band (the host engine's own channel). */
#define POLR_COMM_ID_BYTES 128
typedef struct polr_comm polr_comm;
int polr_comm_get_unique_id(void *id /* POLR_COMM_ID_BYTES */);
int polr_comm_create(polr_ctx *ctx, const void *id, int world_size, int rank, polr_comm **out);
int polr_bcast_build(polr_comm *comm, polr_ht **ht, int root, void *stream);
int polr_comm_bytes_broadcast(const polr_comm *comm, uint64_t *bytes);
void polr_comm_destroy(polr_comm *comm);

/* ---------------------------------------------------------------------------------------------
 * Pipeline = what POLARConfig::GenerateJoinOrders produces (src/parallel/polar_config.cpp:19-249):
 * the joins of the run, where each join reads its probe key (a probe-table column, or a build
 * column of an earlier join: left_expression_bindings, :152-229) and the candidate join orders.
 * ------------------------------------------------------------------------------------------- */
#define POLR_MAX_PREDS 4 /* non-equality conditions per join */
typedef struct polr_join_desc {
	polr_ht *ht;
	uint32_t n_keys;
	int32_t key_src_join[POLR_MAX_KEYS]; /* -1 = probe-table column, j >= 0 = payload column of join j */
	int32_t key_src_col[POLR_MAX_KEYS];
	/* the join's conditions other than equalities (JoinCondition::comparison; JoinHashTable::predicates,
	 * join_hashtable.cpp:50-52; RowOperations::Match, row_match.cpp:59-119): `left OP right` with the left side read
	 * like a key (pred_src_*) and the right side a payload column of this join's build side; a NULL on either side
	 * never matches; both sides must have the same width.  The join's output (and its share of the intermediates)
	 * are the pairs that pass. */
	uint32_t n_preds;
	uint32_t pred_op[POLR_MAX_PREDS]; /* POLR_CMP_EQ .. POLR_CMP_GE, POLR_CMP_STR_EQ.  EQ is the verifying comparison of a
	                                     composite key the engine hands over HASHED (an 8-byte key column = its hash of the
	                                     key columns, one EQ condition per column): the way in for composite keys whose
	                                     value ranges do not pack into 64 bits */
	int32_t pred_src_join[POLR_MAX_PREDS];
	int32_t pred_src_col[POLR_MAX_PREDS];
	uint32_t pred_build_col[POLR_MAX_PREDS];
} polr_join_desc;

int polr_pipeline_create(polr_ctx *ctx, const polr_col *probe_cols, uint32_t n_probe_cols, uint64_t n_probe_rows,
                         const polr_join_desc *joins, uint32_t k, const int32_t *paths /* n_paths x k */,
                         uint32_t n_paths, polr_pipeline **out);
/* A pipeline whose SOURCE is the output of another pipeline, gathered on the device: the probe-side hand-over between two
 * pipelines of one query.  A pipeline holds at most POLR_MAX_JOINS joins; the reference runs a longer query as several
 * pipelines, the rows one emits being the source of the next.  `o` is an output a materialising run has filled; cols[i] names
 * a column of its pipeline as polr_ht_from_output does, and becomes PROBE COLUMN i of the new pipeline.  joins, k, paths and
 * n_paths are exactly polr_pipeline_create's: key_src_join = -1 (and pred_src_join = -1) now names a gathered column.
 * Rows and row ids: the new pipeline has ONE PROBE ROW PER OUTPUT ROW of `o`, in the order of polr_out_fetch_ids /
 * polr_out_materialize (chunk-major, partially filled chunks included).  Probe row r of the new pipeline is output row r of
 * `o`; so slot 0 of any output of the new pipeline indexes polr_out_fetch_ids(o), whose slots in turn name the probe row and
 * the build rows of the first pipeline: row ids compose across the cut through that one array, and through nothing else.
 * Columns: column i has the width and the POLR_COL_SIGNED flag of its source; every column gets a validity array gathered
 * from its source's (all rows valid where the source has none); the cell of a NULL row is zero and the source cell of a NULL
 * row is never read; the same source column may be named more than once.  At most 66 columns.
 * VARCHAR columns (width 16): the cells are normalised exactly as polr_out_materialize_strings normalises them (inline
 * strings zero-padded, NULL rows all-zero) and the long strings' bytes go into a packed heap THE NEW PIPELINE OWNS, one per
 * such column; the column counts as rebased, so a later polr_pipeline_set_probe_heaps on it is refused.  A source column
 * the library uploaded whose heap never came is POLR_E_INVALID once a long non-NULL cell is among the output rows (decided by
 * the measuring pass, before any pointer is followed).
 * Ownership: when the call returns the new pipeline shares nothing with `o`, with o's pipeline, with that pipeline's tables or
 * with a caller's POLR_COL_DEVICE memory -- all of those may be destroyed.  It borrows the tables named in `joins`, as every
 * pipeline does.  All cells, all validity arrays and the gather's descriptors are ONE allocation; polr_device_bytes_live()
 * accounts for every byte.
 * Afterwards the pipeline is an ordinary one: polr_pipeline_set_selection, the four scan-filter calls (also over columns that
 * came from different tables of the first pipeline), LIP, polr_pipeline_update_probe, polr_out_create, every run kind, every
 * sink, polr_ht_from_output and polr_pipeline_from_output of its outputs.
 * Refusals -- nothing is enqueued beyond the output's own statistics, *out = NULL, polr_device_bytes_live() as before --
 * checked in this order:
 *   1. POLR_E_INVALID      NULL o, out, cols, joins or paths
 *   2. POLR_E_INVALID      n_cols == 0
 *   3. POLR_E_UNSUPPORTED  more than 66 columns
 *   4. POLR_E_INVALID      an output with a fused GROUP BY sink (it holds group cells, no row ids)
 *   5. POLR_E_INVALID      a column reference out of range (the first one, in the order of cols)
 *   6. POLR_E_UNSUPPORTED  an output of 2^32 - 16 rows or more (the bound of polr_pipeline_create)
 *   7. every refusal of polr_pipeline_create over the gathered columns, with its own code and message: k outside
 *      1..POLR_MAX_JOINS (nine joins), n_paths outside 1..POLR_MAX_PATHS, a table that is not finalized, a path that is no
 *      permutation or probes a join before the one that provides its key, a key or condition column out of range or of the
 *      wrong width, ...
 * (the heap-never-came refusal comes after these and after the measuring passes; it too leaves *out = NULL and the live
 * bytes as before).
 * An output with no rows, or one no materialising run has filled, behaves exactly as polr_pipeline_create with
 * n_probe_rows = 0: a valid pipeline of zero probe rows and zero tuples, planned and launched like any other (the same
 * polr_pipeline_launch_info); there is no row to select, probe or emit, and polr_pipeline_update_probe of a single row is
 * refused as it is there.
 * Stream: the gather runs on `stream` (NULL: the context's); the call returns when the pipeline is complete (it needs the row
 * count on the host, and with a VARCHAR column the heap totals).
 * Not provided: sinks that address columns of an EARLIER pipeline through composed row ids -- select-list columns are carried
 * forward as columns instead, and a fan-out join copies a string once per output row, as polr_out_materialize_strings does;
 * zero-copy probe columns (views of the first pipeline's tables); more than POLR_MAX_JOINS joins in one pipeline; routing
 * across a cut (each pipeline is multiplexed on its own). */
int polr_pipeline_from_output(polr_out *o, void *stream, const polr_out_col_ref *cols, uint32_t n_cols,
                              const polr_join_desc *joins, uint32_t k, const int32_t *paths /* n_paths x k */,
                              uint32_t n_paths, polr_pipeline **out);
/* The tuples entering the multiplexer, in scan order, when an upstream filter thinned the source
 * chunks (DICTIONARY/sliced vectors, vector.hpp:36-140): sel[i] = probe-table row.  NULL resets
 * to "all rows".  flags: POLR_COL_DEVICE if sel is a device pointer. */
int polr_pipeline_set_selection(polr_pipeline *p, const uint32_t *sel, uint64_t n_sel, uint32_t flags);
/* How the probe kernels of this pipeline are launched (diagnostic): waves per workgroup, workgroups resident per
 * CU (resident kernel), dynamic LDS bytes per workgroup, compiled stage count K and tuple slots W.
 * materialize != 0: the variant that writes row ids (an `out` object is passed to the runs). */
typedef struct polr_launch_info {
	uint32_t waves_per_workgroup, workgroups_per_cu, lds_bytes_per_workgroup, compiled_stages, tuple_slots, n_cus;
	uint32_t flat;            /* 1: counting runs use the flat pipeline (single-key unique-match joins on probe columns) */
	uint32_t lds_tables;      /* bit tables kept in LDS for the whole run */
	uint32_t lds_table_bytes;
	uint32_t pad;
} polr_launch_info;
int polr_pipeline_launch_info(polr_pipeline *p, int materialize, polr_launch_info *info);

/* ---- source side on the device ---------------------------------------
 * PhysicalTableScan with pushed-down table filters: the table is scanned in vectors of `vector_size`
 * rows (STANDARD_VECTOR_SIZE), every vector is thinned to the rows that pass ALL filters, in row order;
 * a vector without a survivor yields no chunk; NULL passes no comparison
 * (src/storage/table/row_group.cpp:316-452 RowGroup::TemplatedScan, src/storage/table/column_segment.cpp:194-475
 * FilterSelection; filter classes src/include/duckdb/planner/filter/{constant,null,conjunction}_filter.hpp).
 * The result -- selection (ascending probe-table rows) and the boundaries of the non-empty chunks --
 * stays in HBM and becomes the pipeline's source (as polr_pipeline_set_selection would install it);
 * multiplexers take the boundaries with polr_mpx_use_scan_chunks.  n_filters == 0: every row passes.
 * A negative constant against an unsigned column is POLR_E_INVALID; OR-conjunctions are not pushed
 * down on this path (POLR_E_UNSUPPORTED would be the caller's: keep them in a host filter).
 * Whichever of the four scan entry points is called, every row's filters are evaluated once: the counting pass keeps
 * one bit per table row in a buffer of the pipeline, the writing pass reads those bits. */
enum {
	POLR_CMP_EQ = 0, POLR_CMP_NE = 1, POLR_CMP_LT = 2, POLR_CMP_GT = 3, POLR_CMP_LE = 4, POLR_CMP_GE = 5,
	POLR_CMP_IS_NULL = 6, POLR_CMP_IS_NOT_NULL = 7,
	/* join conditions only: two columns of 16-byte string cells (string_t) hold the same string.  This is how a VARCHAR
	 * join key arrives: the KEY is the 64-bit hash the engine computes for it anyway (JoinHashTable::Hash,
	 * join_hashtable.cpp:141-155 -- an 8-byte key column on both sides), the strings themselves are this condition --
	 * the hash finds the candidates, the comparison decides, as RowOperations::Match does behind the bucket chain
	 * (row_match.cpp).  The cells' heaps: polr_ht_set_payload_heap / polr_pipeline_set_probe_heap. */
	POLR_CMP_STR_EQ = 8
};
typedef struct polr_scan_filter {
	uint32_t col;     /* probe-table column */
	uint32_t op;      /* POLR_CMP_* (ConstantFilter::comparison_type / IsNullFilter / IsNotNullFilter) */
	int64_t constant; /* ConstantFilter::constant, widened */
} polr_scan_filter;
int polr_pipeline_scan_filter(polr_pipeline *p, void *stream, const polr_scan_filter *filters, uint32_t n_filters,
                              uint32_t vector_size, uint64_t *n_selected, uint64_t *n_chunks);
/* The same scan with LIP (`PRAGMA enable_lip`, lookahead information passing): the source chunks are additionally
 * thinned by the filters of the joins named in `lip_joins` (bit j = join j) before they enter the pipeline --
 * PipelineExecutor::FetchFromSource src/parallel/pipeline_executor.cpp:396-465 probing
 * PhysicalHashJoin::ProbeBloomFilter physical_hash_join.cpp:579-635 for every join with build_bloom_filter
 * (eligibility physical_join.cpp:57-107: one condition, key traced back to a source column).  The reference's filter is
 * a bloom filter sized from a planner estimate; here it is the join's own index (no false positives): a source row
 * survives exactly when its key is not NULL and equals a non-NULL build key of every named join -- the 8-byte key of
 * all ones included, which a repeated-key table keeps beside its slots.  The survivors are a subset of the
 * reference's, the pipeline's output rows are the same.  POLR_E_INVALID for a join that is not keyed by one source
 * column or a mask bit beyond the pipeline's joins, POLR_E_UNSUPPORTED for a join in packed form (its key compared by
 * value or NULL = NULL); a refused call leaves the scan result before it in place. */
int polr_pipeline_scan_filter_lip(polr_pipeline *p, void *stream, const polr_scan_filter *filters, uint32_t n_filters,
                                  uint32_t lip_joins, uint32_t vector_size, uint64_t *n_selected, uint64_t *n_chunks);
/* The same scan with pushed-down VARCHAR constant comparisons.  The reference pushes =, <, >, <=, >= against a VARCHAR
 * constant into the table scan (FilterCombiner::GenerateTableScanFilters, src/optimizer/filter_combiner.cpp:391-398),
 * rewrites prefix(col, 'x') and col LIKE 'abc%...' into col >= 'abc' AND col < 'abd' plus IS NOT NULL (:426-485), and
 * evaluates them on string_t (ColumnSegment::FilterSelection, src/storage/table/column_segment.cpp:435-442).  An engine
 * hands over its TableFilterSet as it is: a ConstantFilter whose Value is a VARCHAR becomes {col, op, 0, bytes, length}.
 *  - A comparison on a column of 16-byte string cells compares the row's string with the constant as
 *    StringComparisonOperators do (comparison_operators.hpp:157-227): memcmp over the shorter length, bytes unsigned, on a
 *    tie the shorter string is the smaller; equal means same length and same bytes.  '\0' and 0x80-0xFF are ordinary
 *    bytes; the padding of an inline cell and the pointer of a long one play no part.  str == NULL with str_len == 0 is
 *    the empty string, which is not NULL.  The constant's bytes are host memory and are copied by the call.
 *  - A NULL row passes no comparison, not even <>; its cell is never read.  IS NULL / IS NOT NULL read the validity only.
 *  - Filters are AND-ed; several may name the same column (the LIKE range); filters on integer columns (`constant`, as
 *    polr_scan_filter) and the LIP mask mix freely with the VARCHAR ones.  With no 16-byte column compared the call is
 *    polr_pipeline_scan_filter_lip.  Row order, skipped empty vectors, chunk boundaries, the installation as the
 *    pipeline's source and the settling of a re-scan are those of polr_pipeline_scan_filter.
 *  - POLR_E_INVALID: str == NULL with str_len > 0; a non-NULL str against a column that is not 16 bytes wide;
 *    POLR_CMP_STR_EQ or any code above POLR_CMP_IS_NOT_NULL; and everything polr_pipeline_scan_filter_lip refuses so.
 *    POLR_E_UNSUPPORTED: a constant longer than POLR_MAX_FILTER_STRING bytes; more than 8 filters.
 *  - The heaps: as for polr_out_aggregate_hashed_str.  A compared column the library uploaded whose heap never came
 *    (polr_pipeline_set_probe_heaps) may hold inline strings only: the call first counts its non-NULL cells longer than 12
 *    bytes, reading length words only, and any such cell is POLR_E_INVALID before a kernel that follows a pointer is
 *    enqueued.  The cells of a POLR_COL_DEVICE column point into HBM by contract.
 *  - A refused call enqueues no scan and leaves the scan result before it in place.
 * OR-conjunctions, IN lists and LIKE beyond the pushed prefix range: polr_pipeline_scan_filter_expr below; collations
 * stay with the engine's own filter. */
#define POLR_MAX_FILTER_STRING 4096
typedef struct polr_scan_filter_str {
	uint32_t col;      /* probe-table column */
	uint32_t op;       /* POLR_CMP_EQ .. POLR_CMP_IS_NOT_NULL */
	int64_t constant;  /* integer column: as polr_scan_filter */
	const void *str;   /* VARCHAR column (width 16): the constant's bytes (host memory, copied by the call) */
	uint64_t str_len;  /* may be 0 (the empty string, which is not NULL) */
} polr_scan_filter_str;
int polr_pipeline_scan_filter_str(polr_pipeline *p, void *stream, const polr_scan_filter_str *filters, uint32_t n_filters,
                                  uint32_t lip_joins, uint32_t vector_size, uint64_t *n_selected, uint64_t *n_chunks);
/* The same scan with a whole boolean expression over the probe table's columns: what the reference evaluates in a
 * PhysicalFilter between the table scan and the first multiplexed join (OR-conjunctions, NOT, IN lists, LIKE beyond the
 * pushed prefix range).  The expression arrives in postfix order: a leaf (POLR_FX_CMP, _IN, _LIKE) pushes one value,
 * POLR_FX_NOT replaces the top, POLR_FX_AND / _OR pop two and push one; it must leave exactly one value.  n_nodes == 0:
 * every row passes.
 *  - SQL three-valued logic, as the reference's ExpressionExecutor evaluates a WHERE: NOT NULL = NULL; NULL AND FALSE =
 *    FALSE, NULL AND TRUE = NULL; NULL OR TRUE = TRUE, NULL OR FALSE = NULL.  A row passes when the root is TRUE, not when
 *    it is NULL.  A CMP, IN or LIKE leaf on a NULL row is NULL and the row's cell is never read; IS NULL / IS NOT NULL read
 *    the validity only and are never NULL.
 *  - POLR_FX_CMP is exactly one filter of polr_pipeline_scan_filter_str: an integer column compares `constant`, a column of
 *    16-byte string cells compares the string (csrc/polr_strcmp.h).  n_values 1; 0 for IS [NOT] NULL.
 *  - POLR_FX_IN is true when the row's value equals one of its n_values >= 1 members: integer members as CMP EQ compares,
 *    VARCHAR members in length and every byte.  A NULL member is not offered; NOT IN is POLR_FX_NOT over it.  (The
 *    reference turns an IN list of fewer than 6 members into an OR of equalities and a longer constant list into a MARK
 *    join in front of the filter, src/optimizer/in_clause_rewriter.cpp:42-106: this leaf stands for both.)
 *  - POLR_FX_LIKE (16-byte string cells only) matches the row's string against the pattern values[first_value], in bytes:
 *    '%' matches any run of bytes, none included; '_' exactly one BYTE (TemplatedLikeOperator advances one byte,
 *    src/function/scalar/string/like.cpp:22-65); every other byte matches itself.  There is no ESCAPE clause: a backslash
 *    is an ordinary byte, and a pattern that holds a '\0' byte -- the escape character the reference binds a LIKE without
 *    ESCAPE with -- is POLR_E_UNSUPPORTED.  NOT LIKE is POLR_FX_NOT over it.  This covers what the reference's optimizer
 *    turns into contains, suffix, prefix and =; ILIKE, ESCAPE, SIMILAR TO and regular expressions stay with the engine.
 *  - lip_joins, vector_size, stream, n_selected, n_chunks, row order, skipped empty vectors, chunk boundaries, the
 *    installation as the pipeline's source, polr_pipeline_fetch_scan and the settling against the scan before or after are
 *    those of polr_pipeline_scan_filter_str; so are the heaps: a column the library uploaded whose heap never came and that
 *    holds a non-NULL cell longer than 12 bytes is POLR_E_INVALID from the pass over the length words, before a kernel that
 *    follows a pointer is enqueued (only columns some CMP, IN or LIKE leaf reads are looked at).
 *  - POLR_E_INVALID: stack underflow, more or fewer than one value left, an unknown kind or op; a value range outside
 *    `values`; col beyond the probe columns; str != NULL against an integer column, str == NULL with str_len > 0; LIKE on
 *    an integer column or with n_values != 1; IN with n_values == 0; CMP with another n_values than above; a negative
 *    constant against an unsigned column; and everything polr_pipeline_scan_filter_lip refuses so.
 *    POLR_E_UNSUPPORTED: more than POLR_MAX_FILTER_NODES nodes, an operand stack deeper than POLR_MAX_FILTER_DEPTH, more
 *    than POLR_MAX_FILTER_VALUES values, more than POLR_MAX_FILTER_BYTES bytes of VARCHAR constants and patterns together,
 *    one constant longer than POLR_MAX_FILTER_STRING, more than 8 distinct columns, a NUL byte in a pattern.
 *  - A refused call enqueues nothing and leaves the scan result before it in place.  nodes, values and the values' bytes
 *    are host memory and are copied by the call. */
#define POLR_MAX_FILTER_NODES 64    /* nodes of one expression */
#define POLR_MAX_FILTER_DEPTH 32    /* operand stack depth the postfix order may reach */
#define POLR_MAX_FILTER_VALUES 64   /* constants of one call (comparison constants, IN members, patterns) */
#define POLR_MAX_FILTER_BYTES 16384 /* bytes of all VARCHAR constants and patterns of one call together */
enum { POLR_FX_CMP = 0, POLR_FX_IN = 1, POLR_FX_LIKE = 2, POLR_FX_NOT = 3, POLR_FX_AND = 4, POLR_FX_OR = 5 };
typedef struct polr_filter_value {
	int64_t constant; /* integer column: as polr_scan_filter */
	const void *str;  /* VARCHAR column (width 16): the constant's / member's / pattern's bytes, as polr_scan_filter_str */
	uint64_t str_len;
} polr_filter_value;
typedef struct polr_filter_node {
	uint32_t kind;        /* POLR_FX_* */
	uint32_t col;         /* leaves: probe-table column */
	uint32_t op;          /* POLR_FX_CMP: POLR_CMP_EQ .. POLR_CMP_IS_NOT_NULL */
	uint32_t first_value; /* leaves: values[first_value .. first_value + n_values) */
	uint32_t n_values;    /* CMP: 1 (0 for IS [NOT] NULL); IN: 1 or more; LIKE: 1, the pattern */
	uint32_t pad;
} polr_filter_node;
int polr_pipeline_scan_filter_expr(polr_pipeline *p, void *stream, const polr_filter_node *nodes, uint32_t n_nodes,
                                   const polr_filter_value *values, uint32_t n_values, uint32_t lip_joins,
                                   uint32_t vector_size, uint64_t *n_selected, uint64_t *n_chunks);
/* read the scan result back (tests): sel[n_selected], chunk_offsets[n_chunks + 1]; either may be NULL */
int polr_pipeline_fetch_scan(polr_pipeline *p, uint32_t *sel, uint64_t *chunk_offsets);
/* Refresh the cells of probe column `col` in place (a new DataChunk arriving at the operator-level
 * drop-in, PhysicalHashJoin::Execute physical_hash_join.cpp:637-681): n_rows <= the row count the
 * pipeline was created with; becomes the new tuple count.  Only for columns the library owns (created
 * from host pointers). */
int polr_pipeline_update_probe(polr_pipeline *p, uint32_t col, const void *data, const uint8_t *valid,
                               uint64_t n_rows);
void polr_pipeline_destroy(polr_pipeline *p);

/* ---------------------------------------------------------------------------------------------
 * Output: a stream of fixed-capacity chunks of row ids (late materialisation).  Slot 0 = probe
 * row, slot 1+j = build row of join j in the ORIGINAL join order, i.e. PhysicalAdaptiveUnion
 * (src/execution/operator/polr/physical_adaptive_union.cpp:37-76) is already applied.
 * ------------------------------------------------------------------------------------------- */
/* max_chunks must cover outputs/chunk_capacity plus one partially filled chunk per emitting wave (at most the
 * resident waves of the device, <= 8192); too small -> POLR_E_OVERFLOW with exact counters, retry larger. */
int polr_out_create(polr_pipeline *p, uint32_t chunk_capacity, uint64_t max_chunks, polr_out **out);
/* Asynchronous on `stream`.  A run that is given this output afterwards is ordered behind the reset on whatever stream
 * it runs (a run on the same stream by the stream, another by an event): a reset never lands behind the run it precedes. */
int polr_out_reset(polr_out *o, void *stream);
int polr_out_stats(polr_out *o, void *stream, uint64_t *n_rows, uint64_t *n_chunks, uint32_t *overflowed);
/* compacted ids to the host: dst[n_rows][1+k] (slot-major per row) */
int polr_out_fetch_ids(polr_out *o, void *stream, uint32_t *dst, uint64_t dst_rows);
/* Gather one output column for every output row (RowOperations::Gather, row_gather.cpp:16-173 /
 * DataChunk::Slice for probe columns): src_join = -1 -> probe column src_col, else payload column
 * src_col of join src_join.  dst_data/dst_valid are host or device pointers (dst_flags). */
int polr_out_materialize(polr_out *o, void *stream, int32_t src_join, uint32_t src_col, void *dst_data,
                         uint8_t *dst_valid, uint64_t dst_rows, uint32_t dst_flags);
/* A VARCHAR column of the output as strings the caller can read: complete string_t cells plus a packed heap of the long
 * strings' bytes, both in the DESTINATION's address space (RowOperations::Gather for string_t, row_gather.cpp:47-86).
 * polr_out_materialize copies a 16-byte cell as it is, so once the column's heap lives on the device (polr_ht_set_payload_heaps
 * / polr_pipeline_set_probe_heaps, a POLR_COL_DEVICE column, a table received over polr_bcast_build) its long cells carry
 * device pointers; this call is the one that hands such a column back.
 *  - Rows and their order are those of polr_out_fetch_ids and polr_out_materialize (chunk-major); src_join / src_col as for
 *    polr_out_materialize.  dst_flags & POLR_COL_DEVICE: dst_cells, dst_valid and dst_heap are device memory, otherwise host
 *    memory.  dst_valid may be NULL.
 *  - Cells: dst_cells[i] is a complete string_t.  A non-NULL string of at most 12 bytes: its length, its bytes, then ZERO
 *    padding whatever the source cell's padding held (the reference compares inline cells as words).  A longer one: its
 *    length, its first four bytes, and the pointer (uint64_t)dst_heap + offset.  A NULL row: validity 0 and an all-zero
 *    cell; it takes no heap bytes and its source cell is never read.
 *  - Heap: packed.  The offset of row i is the sum of the lengths of the non-NULL rows before i that are longer than 12
 *    bytes: no gaps, no terminators, no sharing -- two output rows that name the same build row get a copy each.
 *    *heap_used is the exact total, 64-bit throughout (a chunk's total may exceed 2^32), and is always set (0 by a call
 *    that is refused with POLR_E_INVALID).
 *  - heap_cap < *heap_used: POLR_E_OVERFLOW with *heap_used exact and dst_cells, dst_valid, dst_heap untouched -- one retry
 *    with heap_cap = *heap_used succeeds.  dst_heap == NULL with heap_cap == 0 is the sizing call; it succeeds outright
 *    when no output row is long (all inline, all NULL, or no rows -- also an output that no materialising run has filled).
 *  - POLR_E_INVALID, nothing written: a column that is not 16 bytes wide; dst_rows below the output's rows; NULL dst_cells
 *    with rows to write; dst_heap == NULL with heap_cap > 0; an output with a fused sink (it holds no row ids).  A column
 *    the library uploaded whose heap never came and that has a non-NULL cell longer than 12 bytes among the output rows:
 *    POLR_E_INVALID as for polr_out_aggregate_string, found by the measuring pass, which reads length words only and never
 *    follows a pointer; such a column holding only inline strings works without a heap.
 *  - Two passes over the output chunks: one measures (row id, validity and length word per row; one read-back of the
 *    total decides overflow before anything is written), one writes.  The call returns after the destination is complete.
 *    While it runs it holds scratch of 8 bytes per output row plus 16 bytes per output chunk and, for a host destination,
 *    the staged cells (16 bytes per row), validity (1) and heap (*heap_used); all freed before it returns.
 * Not provided: one heap copy shared by the output rows of one source row; compressed or dictionary output (the code
 * column through polr_out_materialize plus polr_ht_fetch_dictionary already serves that). */
int polr_out_materialize_strings(polr_out *o, void *stream, int32_t src_join, uint32_t src_col, void *dst_cells,
                                 uint8_t *dst_valid, uint64_t dst_rows, void *dst_heap, uint64_t heap_cap,
                                 uint64_t *heap_used, uint32_t dst_flags);

/* ---- sink side on the device -------------------------------------------
 * PhysicalUngroupedAggregate over the pipeline's output (src/execution/operator/aggregate/
 * physical_ungrouped_aggregate.cpp): COUNT(*), COUNT(x), SUM(x), MIN(x), MAX(x) over an integer column x of
 * the probe table (src_join = -1) or of a build side, gathered by the output row ids and reduced on the
 * device -- no column is materialised, only the results leave.  NULLs take no part; SUM is exact in 128 bits
 * (DuckDB: SUM(INTEGER|BIGINT) -> HUGEINT, sum.cpp:113-144) and, like MIN / MAX, NULL over no rows; COUNT is
 * never NULL.  The output object must have been filled by a materialising run (polr_probe_rounds / polr_mpx_run*
 * with an `out`).  VARCHAR / unsigned 64-bit columns: POLR_E_UNSUPPORTED.  An argument that is a product, sum or
 * difference of two columns: the *_expr forms below. */
enum { POLR_AGG_COUNT_STAR = 0, POLR_AGG_COUNT = 1, POLR_AGG_SUM = 2, POLR_AGG_MIN = 3, POLR_AGG_MAX = 4 };
typedef struct polr_agg_spec {
	uint32_t fn;       /* POLR_AGG_* */
	int32_t src_join;  /* -1 = probe-table column, j >= 0 = payload column of join j (ignored for COUNT(*)) */
	uint32_t src_col;
} polr_agg_spec;
typedef struct polr_agg_value {
	int64_t lo, hi;    /* the value as a two's complement 128-bit integer (hi:lo) */
	uint64_t count;    /* rows that took part */
	uint32_t is_null;
	uint32_t pad;
} polr_agg_value;
int polr_out_aggregate(polr_out *o, void *stream, const polr_agg_spec *specs, uint32_t n_aggs,
                       polr_agg_value *results);
/* The same aggregates GROUPed BY up to 3 integer columns with small dense domains -- the case the reference
 * plans as PhysicalPerfectHashAggregate (src/execution/operator/aggregate/physical_perfecthash_aggregate.cpp:
 * every group column has a known [min, max] from its statistics; SSB Q4.x: GROUP BY d_year, c_nation).  Group
 * g = mixed-radix number of the key offsets, ((k0 - min0) * n1 + (k1 - min1)) * n2 + ...; results[g * n_aggs + a];
 * a group no row fell into has count 0 (COUNT) / is_null (SUM, MIN, MAX) and is simply absent from the
 * reference's result.  Rows whose group key is NULL or outside its domain are not aggregated; *n_dropped (may
 * be NULL) counts them (the caller sizes the domains from the build columns' statistics, so normally 0).
 * At most 2^20 groups. */
typedef struct polr_group_key {
	int32_t src_join;   /* -1 = probe-table column, j >= 0 = payload column of join j */
	uint32_t src_col;
	int64_t min_value;
	uint32_t n_values;  /* max - min + 1 */
	uint32_t pad;
} polr_group_key;
int polr_out_aggregate_grouped(polr_out *o, void *stream, const polr_group_key *keys, uint32_t n_keys,
                               const polr_agg_spec *specs, uint32_t n_aggs, polr_agg_value *results,
                               uint64_t n_groups, uint64_t *n_dropped);
/* The general GROUP BY sink -- group columns of ANY integer domain (what the reference plans as PhysicalHashAggregate,
 * src/execution/operator/aggregate/physical_hash_aggregate.cpp, when the columns' statistics do not allow the perfect-hash
 * form): a hash table of groups on the device, NULL a group value of its own (group_nulls: bit c = column c is NULL; its
 * group_keys entry is then 0).  cols: src_join / src_col of polr_group_key (min_value, n_values ignored).  The groups come
 * back in no particular order: group_keys[g * n_cols + c], results[g * n_aggs + a], *n_groups of them; POLR_E_OVERFLOW
 * (with *n_groups = what was found until then) when there are more than max_groups. */
int polr_out_aggregate_hashed(polr_out *o, void *stream, const polr_group_key *cols, uint32_t n_cols,
                              const polr_agg_spec *specs, uint32_t n_aggs, uint64_t max_groups, int64_t *group_keys,
                              uint32_t *group_nulls, polr_agg_value *results, uint64_t *n_groups);
/* The general GROUP BY sink with VARCHAR group columns (SSB: GROUP BY d_year, c_nation; c_city, s_city, d_year; d_year,
 * p_brand).  Each of the 1..3 group columns is taken for what it is: a width-16 column holds string_t cells (see "VARCHAR
 * columns" below) and groups by the string's VALUE -- two rows are in one group iff their lengths and all their bytes are
 * equal (bytes unsigned; \0 and 0x80-0xFF are ordinary bytes; the empty string is a group and is not NULL; the padding of
 * an inline cell and the heap address of a long string play no part) --; a column of up to 8 bytes groups as in
 * polr_out_aggregate_hashed (unsigned 64-bit: POLR_E_UNSUPPORTED).  NULL is a group value of its own per column; the cell of
 * a NULL row is never read.  The aggregates are those of polr_out_aggregate over integer columns.  With integer columns only
 * the call IS polr_out_aggregate_hashed (and *str_used = 0).
 * Results as for polr_out_aggregate_hashed, except that for a VARCHAR column group_keys[g * n_cols + c] is the byte offset
 * in str_bytes of the STRING RECORD of the group's string (0, and to be ignored, when the column's group_nulls bit is set).
 * A string record is {uint32 length (little endian), bytes}; records follow each other without padding, and none is written
 * unless all fit.  It is the one format in which strings leave the device, here and in polr_ht_fetch_dictionary[_codes]
 * below.  *str_used = the bytes the records take.  str_cap < *str_used: POLR_E_OVERFLOW with
 * *n_groups and *str_used exact and group_keys, group_nulls, results and str_bytes untouched -- one retry with str_cap =
 * *str_used succeeds.  More than max_groups groups: POLR_E_OVERFLOW as for polr_out_aggregate_hashed, *str_used = 0.
 * The strings of a VARCHAR column longer than 12 bytes are read through the cells' pointers, so they must be on the device:
 * the column's heap was handed over (polr_ht_set_payload_heaps / polr_pipeline_set_probe_heaps), or the column lives in
 * the caller's device memory (POLR_COL_DEVICE: its cells point into HBM by contract).  For a column the library uploaded
 * whose heap it never got, the call first counts the non-NULL cells longer than 12 bytes among the output rows (reading
 * their length word and nothing else); any such cell: POLR_E_INVALID, before a kernel that follows a pointer is enqueued.
 * All-inline columns need no heap.  MIN / MAX of a VARCHAR per group is not provided.  polr_out_aggregate_grouped and
 * polr_out_fuse_grouped take a VARCHAR column of a BUILD side through its code column (polr_ht_encode_dictionary below);
 * probe-side VARCHAR group columns stay with this sink. */
int polr_out_aggregate_hashed_str(polr_out *o, void *stream, const polr_group_key *cols, uint32_t n_cols,
                                  const polr_agg_spec *specs, uint32_t n_aggs, uint64_t max_groups, int64_t *group_keys,
                                  uint32_t *group_nulls, polr_agg_value *results, uint64_t *n_groups, uint8_t *str_bytes,
                                  uint64_t str_cap, uint64_t *str_used);
/* Cell width in bytes of the column (src_join, src_col) as the sinks address it (src_join = -1: probe column): 16 = a VARCHAR
 * column of string_t cells, 1 / 2 / 4 / 8 an integer one.  How a caller of polr_out_aggregate_hashed_str that did not create
 * the tables itself (a broadcast copy, polr_ht_alloc_like) tells which group_keys entries are offsets. */
int polr_out_column_width(polr_out *o, int32_t src_join, uint32_t src_col, uint32_t *width);
/* ---- aggregate arguments that are `left OP right` ------------------------------------------------------------------
 * SSB flight 1 is SUM(lo_extendedprice * lo_discount), flight 4 SUM(lo_revenue - lo_supplycost): the argument of an
 * aggregate is an expression.  The reference evaluates it in a projection under PhysicalUngroupedAggregate /
 * PhysicalPerfectHashAggregate / PhysicalHashAggregate; polr_agg_expr stands for the BoundFunctionExpression (+, -, *) that
 * is the child of a BoundAggregateExpression, with BoundReferenceExpression children.  Here the sink kernels gather both
 * operands by the row ids they read anyway -- no column is materialised -- under the reference's semantics
 * (src/include/duckdb/common/operator/{add,subtract,multiply}.hpp):
 *  - op = POLR_ARG_COLUMN: the argument is column (src_join[0], src_col[0]); the remaining fields are ignored and the answer
 *    is that of the call without _expr on the same output.
 *  - otherwise the argument is (src_join[0], src_col[0]) OP (src_join[1], src_col[1]); each operand an integer column of the
 *    probe table (src_join = -1) or of a build side, of up to 8 bytes, signed if 8 (else POLR_E_UNSUPPORTED); the two may
 *    come from different sources.
 *  - result_width (1, 2, 4 or 8 bytes) and result_flags (POLR_COL_SIGNED; an 8-byte result must be signed, else
 *    POLR_E_UNSUPPORTED) are the type the reference's binder gave the expression (typeof(expr)).  It must hold the whole
 *    range of both operand types -- the implicit casts the binder adds are lossless --, else POLR_E_INVALID.
 *  - a row whose left or right operand is NULL has a NULL argument: it takes no part in COUNT, SUM, MIN or MAX and cannot
 *    overflow.
 *  - EVERY output row with two non-NULL operands is checked, rows that polr_out_aggregate_grouped_expr drops for their
 *    group key included (the projection runs before the GROUP BY): when the exact result of some row lies outside the
 *    result type the call returns POLR_E_RANGE, *n_out_of_range (may be NULL) is the exact number of such (row, aggregate)
 *    arguments over all aggregates of the call, every result buffer (results, group_keys, group_nulls, str_bytes) and
 *    *n_groups / *n_dropped are as they were, and polr_last_error names the first aggregate index with such a row and
 *    the count.  On success *n_out_of_range = 0.
 * Within range the value is an ordinary signed 64-bit cell: sums are exact in 128 bits, results as for the plain calls.
 * Not provided: constant operands, nested expressions, division, DOUBLE / HUGEINT results; polr_out_fuse_grouped takes
 * plain columns only. */
enum { POLR_ARG_COLUMN = 0, POLR_ARG_ADD = 1, POLR_ARG_SUB = 2, POLR_ARG_MUL = 3 };
typedef struct polr_agg_expr {
	uint32_t fn;           /* POLR_AGG_* (COUNT(*): everything else is ignored) */
	uint32_t op;           /* POLR_ARG_* */
	int32_t src_join[2];   /* left, right operand: -1 = probe-table column, j >= 0 = payload column of join j */
	uint32_t src_col[2];
	uint32_t result_width; /* bytes */
	uint32_t result_flags; /* POLR_COL_SIGNED */
} polr_agg_expr;
int polr_out_aggregate_expr(polr_out *o, void *stream, const polr_agg_expr *specs, uint32_t n_aggs, polr_agg_value *results,
                            uint64_t *n_out_of_range);
int polr_out_aggregate_grouped_expr(polr_out *o, void *stream, const polr_group_key *keys, uint32_t n_keys,
                                    const polr_agg_expr *specs, uint32_t n_aggs, polr_agg_value *results, uint64_t n_groups,
                                    uint64_t *n_dropped, uint64_t *n_out_of_range);
/* integer and VARCHAR group columns, as polr_out_aggregate_hashed_str */
int polr_out_aggregate_hashed_expr(polr_out *o, void *stream, const polr_group_key *cols, uint32_t n_cols,
                                   const polr_agg_expr *specs, uint32_t n_aggs, uint64_t max_groups, int64_t *group_keys,
                                   uint32_t *group_nulls, polr_agg_value *results, uint64_t *n_groups, uint8_t *str_bytes,
                                   uint64_t str_cap, uint64_t *str_used, uint64_t *n_out_of_range);
/* The same GROUP BY FUSED into the run (SSB-skew Q4.1 as shipped: benchmark/ssb-skew/queries/q4-1.sql): an output object
 * with a fused sink makes the pipeline's LAST join fold every surviving tuple into the group cells instead of writing its
 * row ids -- nothing of the join result is written or read back.  For FLAT pipelines whose joins are all perfect tables
 * (polr_pipeline_launch_info(p, 1): flat) -- the star joins of SSB; COUNT(*), COUNT and SUM over columns of at most 4
 * bytes, at most 4096 groups; POLR_E_UNSUPPORTED otherwise (then: polr_out_aggregate_grouped over the emitted row ids).
 * Plain columns only: an argument `left OP right` goes to polr_out_aggregate_grouped_expr over the emitted row ids.
 * polr_out_reset zeroes the cells; every run with this `out` adds to them; polr_out_fused_result reads them (results as
 * for polr_out_aggregate_grouped).  keys == NULL un-fuses.  Only the pool launch (polr_mpx_run_resident*,
 * polr_mpx_run_backpressure) fills the cells: polr_probe_rounds, polr_probe_rounds_async, polr_mpx_run and
 * polr_mpx_run_many return POLR_E_UNSUPPORTED for an `out` with a fused sink and enqueue nothing. */
int polr_out_fuse_grouped(polr_out *o, const polr_group_key *keys, uint32_t n_keys, const polr_agg_spec *specs,
                          uint32_t n_aggs);
int polr_out_fused_result(polr_out *o, void *stream, polr_agg_value *results, uint64_t n_groups, uint64_t *n_dropped);
/* PhysicalUngroupedAggregate FUSED into the run, for ANY pipeline (every JOB query ends in SELECT MIN(a), MIN(b), ...;
 * SSB flight 1 is ungrouped too): an output object with this sink makes the GENERIC pool kernel fold every final tuple
 * into aggregate cells where it would have written the tuple's row ids -- no row id is written, no output has to be sized,
 * no second pass reads the result back.
 *  - polr_out_fuse_aggregate attaches 1..8 aggregates (COUNT(*), COUNT, SUM, MIN, MAX; polr_agg_spec as for
 *    polr_out_aggregate) over integer columns of the probe table or of any build side, of 1, 2, 4 or 8 bytes.  Refused, in
 *    this order: NULL o (POLR_E_INVALID); more than 8 aggregates (POLR_E_UNSUPPORTED); an output that carries a fused sink
 *    already, this one or polr_out_fuse_grouped's -- an output carries at most one of the two (POLR_E_INVALID); then per
 *    aggregate, in order, exactly the column rule of polr_out_aggregate with its wording: an unknown function, a column
 *    out of range (POLR_E_INVALID), a VARCHAR or unsigned 8-byte column (POLR_E_UNSUPPORTED).  A VARCHAR column of a build
 *    side goes through its sorted code column (polr_ht_encode_dictionary_ex with POLR_DICT_SORTED | POLR_DICT_NULL_INVALID:
 *    MIN of the codes is the code of the MIN string; polr_ht_fetch_dictionary_codes turns it back).
 *    specs == NULL or n_aggs == 0 un-fuses: the output collects row ids again.
 *  - any pipeline is accepted.  While the sink is attached an emitting pool launch with this `out` runs on the generic kernel
 *    over the materialising descriptors, also where the pipeline's emitting runs would take the flat kernel;
 *    polr_pipeline_launch_info is not affected.
 *  - the results are those of polr_out_aggregate over the rows the same run would have emitted: NULL arguments take no part,
 *    COUNT is never NULL, SUM / MIN / MAX over no rows are is_null, SUM is exact in 128 bits; routing, the number of
 *    executors and the run kind change nothing.
 *  - every run with this `out` adds to the cells; polr_out_reset returns them to "no rows"; polr_out_fused_aggregate_result
 *    reads them (n_aggs must be the sink's, else POLR_E_INVALID, as is an output without the sink) and may be called
 *    repeatedly.  Only the pool launch fills the cells (polr_mpx_run_resident*, _ranges, _morsels, _stealing,
 *    polr_mpx_run_backpressure): polr_probe_rounds, polr_probe_rounds_async, polr_mpx_run and polr_mpx_run_many return
 *    POLR_E_UNSUPPORTED for such an `out` and enqueue nothing.
 *  - the output holds no row ids: polr_out_fetch_ids, polr_out_materialize*, polr_out_aggregate* (every form),
 *    polr_ht_from_output and polr_pipeline_from_output return POLR_E_INVALID; polr_out_stats reports no rows.
 *  - the SUM cells are exact while fewer than 2^32 tuples have been folded since the last reset: with 2^32 or more and a SUM
 *    in the sink the result call returns POLR_E_RANGE and leaves `results` untouched.
 * Not provided: `left OP right` arguments, VARCHAR arguments (probe-side strings: polr_out_aggregate_string over emitted row
 * ids), GROUP BY (polr_out_fuse_grouped on flat pipelines, polr_out_aggregate_grouped / _hashed elsewhere). */
int polr_out_fuse_aggregate(polr_out *o, const polr_agg_spec *specs, uint32_t n_aggs);
int polr_out_fused_aggregate_result(polr_out *o, void *stream, polr_agg_value *results, uint32_t n_aggs);
/* ---- VARCHAR columns and their sink (every JOB query ends in MIN of a VARCHAR: benchmark/imdb_plan_cost/queries/18a.sql:1-3) --------
 * A width-16 column holds string_t cells (src/include/duckdb/common/types/string_type.hpp:23-28: 4-byte length; up to 12
 * characters inline; longer: a 4-byte prefix and an 8-byte pointer into a string heap).  RowOperations::Gather copies such
 * cells as they are, the pointer staying into the table's heap (row_gather.cpp:47-86).  A column with non-inlined strings
 * needs that heap on the device.  The reference's heaps (StringHeap, a row layout's heap) are lists of blocks: the *_heaps
 * calls take one {base, bytes} range per block, copy every range into HBM and rebase the pointers of the column's cells onto
 * the copies; the heap copy is owned by the table / pipeline.  The contract:
 *  - ranges must be non-empty, non-NULL and disjoint; every non-NULL cell longer than 12 bytes must lie wholly inside one
 *    of them (length and pointer of the cell), else POLR_E_INVALID;
 *  - the cells of NULL rows (column validity 0) are never read -- the reference leaves them uninitialised -- and are
 *    zeroed (an empty string), so no later kernel follows their pointers;
 *  - all or nothing: every cell is checked before any is rewritten; on an error the cells are exactly as they were and
 *    no device heap is kept, so a corrected call may follow;
 *  - once per column: a second call on a column whose cells were rebased returns POLR_E_INVALID and changes nothing;
 *  - a payload column's heap is set before the table is finalized (a perfect table keeps a re-ordered copy of the cells).
 * polr_ht_set_payload_heap / polr_pipeline_set_probe_heap are the same with the one range [heap_base, heap_base +
 * heap_bytes). */
typedef struct polr_heap_range {
	const void *base;
	uint64_t bytes;
} polr_heap_range;
int polr_ht_set_payload_heaps(polr_ht *ht, uint32_t payload_col, const polr_heap_range *ranges, uint32_t n_ranges);
int polr_pipeline_set_probe_heaps(polr_pipeline *p, uint32_t probe_col, const polr_heap_range *ranges, uint32_t n_ranges);
int polr_ht_set_payload_heap(polr_ht *ht, uint32_t payload_col, const void *heap_base, uint64_t heap_bytes);
int polr_pipeline_set_probe_heap(polr_pipeline *p, uint32_t probe_col, const void *heap_base, uint64_t heap_bytes);
/* ---- dictionary codes for VARCHAR build columns (SSB: every grouped query groups by a VARCHAR of a dimension table --
 * c_nation, s_nation, c_city, s_city, p_brand) -----------------------------------------------------------------------
 * A group column that is a payload column of a build side has at most as many distinct values as the build side has
 * rows, and the build side is uploaded once.  polr_ht_encode_dictionary encodes VARCHAR payload column `payload_col` of a
 * table that is NOT YET FINALIZED once per build row, on the device, into dense codes, and appends ONE payload column to
 * the table: index *code_col = the table's payload count before the call, 4 bytes wide, unsigned, no validity array.  From
 * then on it is an ordinary payload column for every consumer -- polr_ht_export / polr_ht_alloc_like, finalize (a perfect
 * table re-orders it with the others), polr_out_materialize, polr_out_column_width (4), join conditions and all sinks:
 * polr_out_aggregate_grouped and polr_out_fuse_grouped group by the strings of a build side through it, with a domain that
 * is tight by construction, and the probe side reads one 4-byte cell per surviving tuple.
 *  - Two rows get the same code iff their strings are equal as for polr_out_aggregate_hashed_str: same length, same bytes;
 *    the padding of an inline cell and the heap address play no part.
 *  - Codes are deterministic: the code of a value is the number of distinct non-NULL values whose first occurrence (lowest
 *    build row, rows as uploaded) comes before its own -- 0 .. *n_codes - 1 in order of first appearance.  Rows whose KEY is
 *    NULL are encoded like any other.
 *  - A NULL row (column validity 0) gets code *n_codes; its cell is never read.  *has_null = 1 iff there is one.  So
 *    n_values = *n_codes + *has_null makes NULL a group of its own (GROUP BY), n_values = *n_codes leaves NULL rows to
 *    *n_dropped of polr_out_aggregate_grouped.
 *  - Refusals, each leaving the table exactly as it was (payload count included): a finalized table (as for
 *    polr_ht_set_payload_heaps), a column that is not 16 bytes wide, a column that is encoded already: POLR_E_INVALID; a
 *    column the library uploaded whose heap never came and that holds a non-NULL cell longer than 12 bytes: POLR_E_INVALID,
 *    found by a pass over the build rows that reads length words only, before any kernel follows a pointer (set the heap,
 *    then encode).  A table that has 62 payload columns already: POLR_E_UNSUPPORTED (polr_ht_export carries 62).  A table
 *    of 0 rows encodes to *n_codes = 0.
 *  - `stream` as for polr_ht_finalize_*; the call waits for the context's own stream first (uploads and heaps went there)
 *    and returns after the codes are complete.  While it runs it holds scratch memory of 36 bytes per slot of a string
 *    table of 2 to 4 slots per build row, plus 8 bytes per build row -- up to about 150 bytes per build row, freed before
 *    it returns: sized for dimension tables; POLR_E_HIP (table untouched) when the device cannot give that much.
 * The table keeps one representative string_t cell per code (pointing into the heap it owns); polr_ht_fetch_dictionary
 * reads them: offsets[c] = byte offset in str_bytes of the string record (polr_out_aggregate_hashed_str above) of code c,
 * c < n_codes; *str_used = the bytes the records take.  str_cap < *str_used or n_offsets < n_codes: POLR_E_OVERFLOW with
 * *str_used exact and offsets / str_bytes untouched -- one retry with *str_used succeeds.  POLR_E_INVALID for a column that
 * is not a code column of this table, a table that was never encoded, and a table made by polr_ht_alloc_like / received
 * by polr_bcast_build (they carry the codes, not the strings: the rank that built the table holds the dictionary).
 *
 * polr_ht_encode_dictionary_ex is the same call with `flags`; flags = 0 IS polr_ht_encode_dictionary, bit for bit, and a
 * column encoded by either call is "encoded already" for both.  A bit other than the two below: POLR_E_INVALID, table
 * untouched.  Refusals, atomicity and the stream rule are those above.
 *  - POLR_DICT_SORTED: the code of a value is the number of distinct non-NULL values of the column that are SMALLER than it
 *    (bytes compared as unsigned, a proper prefix first: the order of polr_out_aggregate_string and of the reference's
 *    string comparison) -- 0 .. *n_codes - 1 ascending with the strings, whatever the order of the build rows, the padding
 *    of inline cells or the heap addresses.  NULL rows still get *n_codes, the largest code.  polr_ht_fetch_dictionary then
 *    returns the strings in ascending order.  What it buys: a result of polr_out_aggregate_grouped / polr_out_fuse_grouped
 *    read in index order is in ORDER BY order of the group columns (NULL last), and MIN / MAX of the column -- per group or
 *    over all rows -- is the integer MIN / MAX of its code column in any sink, one 4-byte read per tuple, and one look-up
 *    per result (polr_ht_fetch_dictionary_codes).  The representative cells are sorted on the device (LDS bitonic tiles of
 *    1024 values, then merge passes; nothing but the counts goes to the host); while the call runs the sort holds 52 more
 *    bytes of scratch per DISTINCT value (two 16-byte records, a copy of the cell, the rank), freed before it returns.
 *    *n_codes <= 1 sorts nothing.
 *  - POLR_DICT_NULL_INVALID: when the source column has a validity array the code column gets a device copy of it (counted
 *    in device_bytes), which travels through finalize, polr_ht_export / polr_ht_alloc_like and polr_bcast_build like any
 *    payload validity.  The cell of a NULL row is still *n_codes (polr_out_materialize reports it as it reports every NULL
 *    cell: validity 0, data 0), but COUNT(col) / MIN / MAX over the code column follow
 *    SQL (NULLs take no part), the perfect-hash sink counts NULL-key rows in *n_dropped as for any NULL group key, and the
 *    hashed sink makes NULL a group of its own.  Without the flag, or for a source column without validity: no validity
 *    array, as above.
 * polr_ht_fetch_dictionary_codes returns the string records of the `n` listed codes, in list order, instead
 * of the whole dictionary: offsets[i] = byte offset of the record of codes[i], duplicates get a record each, *str_used =
 * the bytes the records take.  n = 0: POLR_OK, *str_used = 0.  A listed code >= n_codes (the NULL code is not a string):
 * POLR_E_INVALID, nothing written.  str_cap < *str_used: POLR_E_OVERFLOW with *str_used exact and offsets / str_bytes
 * untouched -- one retry succeeds.  POLR_E_INVALID for the same tables as polr_ht_fetch_dictionary. */
#define POLR_DICT_SORTED       1u
#define POLR_DICT_NULL_INVALID 2u
int polr_ht_encode_dictionary(polr_ht *ht, uint32_t payload_col, void *stream, uint32_t *code_col, uint32_t *n_codes,
                              uint32_t *has_null);
int polr_ht_encode_dictionary_ex(polr_ht *ht, uint32_t payload_col, uint32_t flags, void *stream, uint32_t *code_col,
                                 uint32_t *n_codes, uint32_t *has_null);
int polr_ht_fetch_dictionary(polr_ht *ht, uint32_t code_col, void *stream, uint64_t *offsets, uint64_t n_offsets,
                             uint8_t *str_bytes, uint64_t str_cap, uint64_t *str_used);
int polr_ht_fetch_dictionary_codes(polr_ht *ht, uint32_t code_col, void *stream, const uint32_t *codes, uint64_t n,
                                   uint64_t *offsets, uint8_t *str_bytes, uint64_t str_cap, uint64_t *str_used);
/* ---- dictionary codes for VARCHAR PROBE columns (JOB: title.title, the carried select list of a chained plan) ------
 * polr_pipeline_encode_dictionary encodes VARCHAR probe column `probe_col` of a pipeline on the device and appends ONE
 * probe column to it: index *code_col = the pipeline's probe column count before the call, 4 bytes wide, unsigned.  From
 * then on it is an ordinary integer probe column for every consumer: polr_out_aggregate* in all forms,
 * polr_out_fuse_aggregate and polr_out_fuse_grouped (MIN(varchar) is MIN(code) inside the pool launch, GROUP BY a probe
 * string is GROUP BY its code), polr_out_materialize, polr_out_column_width (4), polr_pipeline_column_stats, the three
 * scan-filter entry points, and polr_pipeline_from_output, which carries it forward as a plain 4-byte column (the strings
 * stay with the pipeline that encoded).
 *  - The code rules are those of polr_ht_encode_dictionary_ex above, word for word, with "table row" for "build row": equal
 *    strings get equal codes; without POLR_DICT_SORTED codes count first appearances by table row, with it they ascend with
 *    the strings; a NULL row gets *n_codes and its cell is never read; POLR_DICT_NULL_INVALID copies the validity array;
 *    the heap-never-came guard (POLR_E_INVALID; polr_pipeline_set_probe_heaps, then encode) runs before any pointer is
 *    followed; 0 rows encode to *n_codes = 0.
 *  - POLR_DICT_SELECTED (this call only; polr_ht_encode_dictionary_ex refuses the bit): only the rows of the selection in
 *    force take part -- what POLR_STATS_SELECTED reads: the result of the last scan filter or polr_pipeline_set_selection;
 *    with no selection the flag means all rows.  A row outside the selection is not read; its code is *n_codes, and with
 *    POLR_DICT_NULL_INVALID it is invalid: the code column then gets a validity array of `valid AND selected`, also when the
 *    source column has none.  *has_null, *n_codes and first appearance speak of the selected rows only; first appearance is
 *    the lowest table row among the selected, whatever the order of the selection, and a row listed twice counts once.  The
 *    string table and every scratch array that need not be indexed by table row are sized by the selected count: 36 bytes
 *    per slot of a table of 2 to 4 slots per SELECTED position plus 4 bytes per selected position, and 4 bytes per table
 *    row (plus what the sort takes per distinct value).  THE CODES HOLD FOR RUNS OVER THAT SELECTION OR A SUBSET OF IT: the
 *    library does not track later changes of the selection -- after a wider one, rows that were outside read as NULL.
 *  - Outputs and multiplexers created before the call stay valid, and a run with them afterwards returns what it returned
 *    before.  The call waits for the context's own stream first and returns after the codes are complete; it must not be
 *    called while a run of the pipeline is in flight.
 *  - Refusals, in this order, each leaving the pipeline exactly as it was (column count included): a flag other than the
 *    three, no such probe column, a column that is not 16 bytes wide, a column that is encoded already, a code column as
 *    source: POLR_E_INVALID; a slot space beyond 32 bits: POLR_E_UNSUPPORTED; then a HIP error (POLR_E_HIP) and the heap
 *    guard (POLR_E_INVALID).
 * polr_pipeline_fetch_dictionary / _codes: the sizing and POLR_E_OVERFLOW protocol of their polr_ht_ twins.  POLR_E_INVALID
 * for a column that is not a code column whose dictionary this pipeline holds.
 * Not provided: dictionaries of probe-side columns shared with a build column; re-encoding after a new selection. */
#define POLR_DICT_SELECTED 4u /* pipeline call only */
int polr_pipeline_encode_dictionary(polr_pipeline *p, uint32_t probe_col, uint32_t flags, void *stream, uint32_t *code_col,
                                    uint32_t *n_codes, uint32_t *has_null);
int polr_pipeline_fetch_dictionary(polr_pipeline *p, uint32_t code_col, void *stream, uint64_t *offsets, uint64_t n_offsets,
                                   uint8_t *str_bytes, uint64_t str_cap, uint64_t *str_used);
int polr_pipeline_fetch_dictionary_codes(polr_pipeline *p, uint32_t code_col, void *stream, const uint32_t *codes, uint64_t n,
                                         uint64_t *offsets, uint8_t *str_bytes, uint64_t str_cap, uint64_t *str_used);
/* MIN / MAX (fn = POLR_AGG_MIN / POLR_AGG_MAX) of a VARCHAR column over the pipeline's output rows, reduced on the
 * device (src/function/aggregate/distributive/minmax.cpp over string_t: bytes compared as unsigned, a proper prefix
 * sorts first; NULLs take no part).  The winning string's bytes go to dst (at most dst_cap of them), *len = its whole
 * length; *is_null = 1 when no row had a non-NULL value.  A column the library uploaded whose heap it never got may hold
 * inline strings only: a non-NULL cell longer than 12 bytes among the output rows is POLR_E_INVALID (found by a pass that
 * reads the cells' length words only), as for polr_out_aggregate_hashed_str. */
int polr_out_aggregate_string(polr_out *o, void *stream, uint32_t fn, int32_t src_join, uint32_t src_col, char *dst,
                              uint32_t dst_cap, uint32_t *len, uint32_t *is_null);
void polr_out_destroy(polr_out *o);

/* ---------------------------------------------------------------------------------------------
 * Probe: RunPath for many routed slices at once (polar_pipeline_executor.cpp:427-538 +
 * PhysicalHashJoin::Execute physical_hash_join.cpp:637-681 + JoinHashTable::Probe /
 * ScanStructure::NextInnerJoin join_hashtable.cpp:396-565 + ProbePerfectHashTable
 * perfect_hash_join_executor.cpp:177-291).  A round = tuples [begin, begin+count) (positions in
 * scan order) sent down join order `path`.  counts[r*k + j] receives the number of tuples the join
 * at position j of that path produced: their sum over j is what RunPath feeds to
 * PhysicalMultiplexer::AddNumIntermediates (:486-487).  out may be NULL (count only).
 * ------------------------------------------------------------------------------------------- */
typedef struct polr_round {
	uint64_t begin;
	uint64_t count;
	uint32_t path;
	uint32_t emit; /* 0: count only (ALTERNATE drops the output of paths != 0, :445-447) */
} polr_round;

int polr_probe_rounds(polr_pipeline *p, void *stream, const polr_round *rounds, uint32_t n_rounds, polr_out *out,
                      uint64_t *counts /* host, n_rounds x k, filled after an internal sync */);
/* asynchronous form: counts stay on the device (n_rounds x k uint64), nothing is synchronised */
int polr_probe_rounds_async(polr_pipeline *p, void *stream, const polr_round *rounds, uint32_t n_rounds,
                            polr_out *out, uint64_t *counts_dev);

/* ---------------------------------------------------------------------------------------------
 * Device-resident multiplexer: PhysicalMultiplexer + RoutingStrategy + the reward update
 * (src/execution/operator/polr/physical_multiplexer.cpp:100-184, routing_strategy.cpp:7-463)
 * evaluated on the device between probe rounds -- by the last workgroup of a path-kernel launch
 * (polr_mpx_run, _run_many) or by the router wave of a resident launch (polr_mpx_run_resident) -- so a
 * whole morsel is routed without a host round trip per routing decision.  Decisions are bit-identical
 * to the host classes in duckdb-polr_amd/host (same source, same double arithmetic, no contraction).
 * ------------------------------------------------------------------------------------------- */
typedef struct polr_mpx_config {
	uint32_t routing;
	uint32_t chunk_size;       /* STANDARD_VECTOR_SIZE of the host engine (1024 in the reference snapshot) */
	double regret_budget;
	uint64_t init_tuple_count;
	uint64_t atc_multiplier;
	uint32_t log_rounds;       /* keep (path, tuples, intermediates) of every routing round */
	uint32_t max_log_rounds;
} polr_mpx_config;

typedef struct polr_mpx_stats {
	uint64_t num_tuples_processed;
	uint64_t num_intermediates;
	uint64_t num_rounds;
	uint64_t input_tuple_count_per_path[POLR_MAX_PATHS];
	double path_resistances[POLR_MAX_PATHS];
	/* tuples produced by the join at position j of join order p, summed over all rounds routed to p
	 * (the per-operator `elements` the reference's profiler reports, query_profiler.cpp:383-404) */
	uint64_t stage_out[POLR_MAX_PATHS][POLR_MAX_JOINS];
} polr_mpx_stats;

int polr_mpx_create(polr_pipeline *p, const polr_mpx_config *cfg, polr_mpx **out);
/* the source chunks are those of the pipeline's polr_pipeline_scan_filter result (boundaries stay in HBM);
 * to be called again after every new scan of the pipeline (a run with a stale attachment is POLR_E_INVALID) */
int polr_mpx_use_scan_chunks(polr_mpx *m);
/* Route and probe source chunks [chunk_begin, chunk_end) (chunk c = tuples [c*chunk_size, ...)
 * unless chunk offsets were set) entirely on the device; asynchronous. */
int polr_mpx_run(polr_mpx *m, void *stream, uint64_t chunk_begin, uint64_t chunk_end, polr_out *out);
/* Several executors at once: ms[i] routes chunks [chunk_begin[i], chunk_end[i]) with its own multiplexer
 * state on its own stream (streams may be NULL: every multiplexer owns one) -- the counterpart of the
 * reference's worker threads, one PipelineExecutor + MultiplexerState each (pipeline.cpp:145-174,
 * pipeline_executor.cpp:28-41).  One host thread pumps all of them, so their routing rounds overlap on the
 * device.  All multiplexers must belong to the same pipeline; `out` (may be NULL) is shared. */
int polr_mpx_run_many(polr_mpx **ms, void **streams, const uint64_t *chunk_begin, const uint64_t *chunk_end,
                      uint32_t n, polr_out *out);
/* The same run as ONE kernel launch ("resident"): the grid is split between the n executors
 * (workgroup % n; with n = 8 one executor per XCD), every executor has a router workgroup that keeps its
 * multiplexer state in LDS and probe workgroups that wait for its rounds on the device -- no launch and no
 * host step between two routing decisions.  Same routing, same results as polr_mpx_run / _run_many with the
 * same chunk ranges.  All executors run on `stream` (NULL: the first multiplexer's).  Asynchronous;
 * polr_mpx_finish(_many) synchronises and reports POLR_E_HIP if the device-side watchdog fired.
 * flags: POLR_RUN_RESET = start from a fresh MultiplexerState (what polr_mpx_reset does, without a launch
 * of its own); POLR_RUN_FINISH = close the run inside the same launch (PushFinalize's FinalizePathRun) and
 * leave the statistics where polr_mpx_finish(_many) picks them up without launching anything.
 * POLR_E_UNSUPPORTED: more than 64 executors / more executors than fit on the device at once. */
#define POLR_RUN_RESET 1u
#define POLR_RUN_FINISH 2u
/* POLR_RUN_SHARE(d): size the grid for 1/d of the device (d = 2..16), so that d resident runs on d streams are
 * co-resident and their rounds overlap (the small exploration rounds of one pass run beside the table-sized
 * round of another) */
#define POLR_RUN_SHARE(d) (((uint32_t)(d) & 0xFFu) << 8)
int polr_mpx_run_resident(polr_mpx **ms, void *stream, const uint64_t *chunk_begin, const uint64_t *chunk_end,
                          uint32_t n, polr_out *out, uint32_t flags);
/* What polr_mpx_run_resident*(ms, .., n, out, flags) would plan for its launch under the context's tuning, by the same
 * steps (diagnostic; launches nothing, changes nothing): the grid, the probe waves, and the numbers that cut a round
 * into units -- a round of more than hi_tuples tuples is cut into units of ceil(tuples / target) tuples, target =
 * max(16, units_x * pool_waves / executors still routing), rounded up to a multiple of gran, at most 65 536; a smaller
 * round into units of hi_unit tuples.  Refuses what the run would refuse (POLR_E_INVALID / POLR_E_UNSUPPORTED). */
typedef struct polr_pool_info {
	uint32_t n_blocks;   /* workgroups of the launch */
	uint32_t pool_waves; /* probe waves */
	uint32_t n_rings;    /* unit rings in use */
	uint32_t mixed;      /* 1: the routers sit in the probe workgroups' first waves */
	uint32_t share;      /* the launch is sized for 1 / share of the device */
	uint32_t units_x, hi_unit, hi_tuples;
	uint32_t gran;       /* 512: the flat pipeline's kernel, 64: the generic one */
	uint32_t flat;
} polr_pool_info;
int polr_mpx_pool_info(polr_mpx **ms, uint32_t n, polr_out *out, uint32_t flags, polr_pool_info *info);
/* The same with a LIST of chunk ranges per executor (range_begin / range_end: [n][ranges_per_executor], 1..8): executor i
 * routes its ranges one after the other with one multiplexer state -- a worker thread that was handed several morsels
 * up front.  Pairing a range from every part of a skewed table per executor evens out what the executors have to do
 * (they finish together) and keeps runs reproducible, which a shared cursor does not. */
int polr_mpx_run_resident_ranges(polr_mpx **ms, void *stream, const uint64_t *range_begin, const uint64_t *range_end,
                                 uint32_t ranges_per_executor, uint32_t n, polr_out *out, uint32_t flags);

/* Morsel-driven variant: the n executors SHARE the chunks [chunk_begin, chunk_end) and pull them `morsel_chunks`
 * chunks at a time from one device-side cursor -- the reference's worker threads pulling morsels from the
 * parallel scan state (a row group = 120 vectors; pipeline.cpp:145-174, table_scan.cpp) -- so a skewed source
 * cannot leave one executor with the expensive end of the table.  Which executor sees which morsel depends on
 * timing (as in the multi-threaded reference): result row set and COUNT(*) are deterministic, per-executor traces
 * and total intermediates are not. */
int polr_mpx_run_resident_morsels(polr_mpx **ms, void *stream, uint64_t chunk_begin, uint64_t chunk_end,
                                  uint32_t morsel_chunks, uint32_t n, polr_out *out, uint32_t flags);
/* Range stealing: as polr_mpx_run_resident -- executor i owns the contiguous chunks [chunk_begin[i], chunk_end[i]), which
 * may be empty -- but it takes them `grant_chunks` chunks at a time, and an executor that has run dry takes the far half
 * (in whole grants) of the executor that has most left, and goes on there with the multiplexer state it has: what the
 * reference's worker threads get from the task scheduler (pipeline.cpp:145-174).  An executor keeps to one stretch of the
 * table as long as it has one; only the tail of the run is rebalanced.
 * Deterministic: row set, COUNT(*), routed tuples.  Not deterministic once a steal has happened: per-executor traces and
 * total intermediates.  While no range holds two grants nobody can steal, and the run is the fixed-range run of
 * polr_mpx_run_resident, decision for decision.
 * POLR_E_INVALID: grant_chunks == 0, a range outside the source, ranges that are not pairwise disjoint (the protocol
 * rests on it).  flags as for polr_mpx_run_resident. */
int polr_mpx_run_resident_stealing(polr_mpx **ms, void *stream, const uint64_t *chunk_begin, const uint64_t *chunk_end,
                                   uint32_t grant_chunks, uint32_t n, polr_out *out, uint32_t flags);
typedef struct polr_steal_stats {
	uint64_t chunks_routed; /* source chunks this executor routed */
	uint64_t chunks_stolen; /* of these, taken from other executors' ranges (always whole grants) */
	uint32_t n_steals, pad;
} polr_steal_stats;
/* this executor's counters of its last run; after polr_mpx_finish(_many); zeros after any run that was not a stealing run */
int polr_mpx_steal_stats(polr_mpx *m, polr_steal_stats *stats);
/* MultiplexerRouting::BACKPRESSURE (src/parallel/pipeline.cpp:147-156, src/parallel/polar_config.cpp:128-147): the
 * reference schedules ONE task per join order over a single shared source state, so the join orders race for the
 * source and the cheaper ones end up with more of it.  ms: one multiplexer per join order of the pipeline (created with
 * POLR_ROUTE_BACKPRESSURE); executor i sends every morsel it pulls (morsel_chunks source chunks at a time; 120 = a row
 * group) down join order i.  Row set and COUNT(*) are deterministic, the split between the orders depends on timing
 * (as in the reference).  Statistics: executor i reports its tuples under path 0 of ITS statistics, its per-stage
 * counters under path i. */
int polr_mpx_run_backpressure(polr_mpx **ms, void *stream, uint64_t chunk_begin, uint64_t chunk_end,
                              uint32_t morsel_chunks, polr_out *out, uint32_t flags);
int polr_mpx_set_chunk_offsets(polr_mpx *m, const uint64_t *offsets, uint64_t n_chunks);
/* fresh MultiplexerState (a new PipelineExecutor / a new pass over the source) */
int polr_mpx_reset(polr_mpx *m, void *stream);
/* bracket every path-kernel launch of polr_mpx_run with HIP events on the launch stream and report
 * the summed device time and launch count since the last call (measurement only) */
int polr_mpx_enable_timing(polr_mpx *m, int enable);
int polr_mpx_kernel_time(polr_mpx *m, double *total_ms, uint64_t *n_launches);
/* PushFinalize's last FinalizePathRun (polar_pipeline_executor.cpp:150-151) + read back */
int polr_mpx_finish(polr_mpx *m, void *stream, polr_mpx_stats *stats);
/* the same for every executor of a polr_mpx_run_many (on the streams the runs used); stats[n] */
int polr_mpx_finish_many(polr_mpx **ms, uint32_t n, polr_mpx_stats *stats);
int polr_mpx_fetch_log(polr_mpx *m, void *stream, uint32_t *path, uint64_t *tuples, uint64_t *intermediates,
                       uint64_t max_rounds, uint64_t *n_rounds);
void polr_mpx_destroy(polr_mpx *m);

#ifdef __cplusplus
}
#endif
#endif
