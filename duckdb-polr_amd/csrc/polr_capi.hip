// duckdb-polr_amd/csrc/polr_capi.hip -- implementation of the C ABI in include/polr_hip.h
// (contexts, build-side residency, pipelines, output chunks, probe launches).
// No CPU fallback anywhere in this file: every entry point either runs on the device or fails.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>

#include <stdlib.h>

#include "polr_internal.h"

void polr_trace_stale(const char *where) {
	static const int enabled = [] {
		const char *v = getenv("POLR_DEBUG_HIP_ERRORS");
		return (v && v[0] && v[0] != '0') ? 1 : 0;
	}();
	static thread_local const char *previous = "(none)";
	if (enabled) {
		const hipError_t e = hipGetLastError(); // (reads and clears)
		if (e != hipSuccess) {
			fprintf(stderr, "[polr] HIP error '%s' was pending on entry of %s; previous entry point: %s\n",
			        hipGetErrorString(e), where, previous);
		}
		previous = where;
	}
}

extern "C" {

int polr_abi_version(void) {
	return POLR_ABI_VERSION;
}

uint64_t polr_device_bytes_live(void) {
	return polr_devbuf_live_bytes.load(std::memory_order_relaxed);
}

int polr_ctx_create(int device_id, polr_ctx **out) {
	POLR_ENTRY();
	if (!out) {
		return POLR_E_INVALID;
	}
	*out = nullptr;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) {
		return POLR_E_NO_DEVICE;
	}
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) {
		return POLR_E_NO_DEVICE;
	}
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
		// the code objects in this library are gfx950 only
		return POLR_E_NO_DEVICE;
	}
	if (hipSetDevice(device_id) != hipSuccess) {
		return POLR_E_NO_DEVICE;
	}
	polr_ctx *ctx = new polr_ctx();
	ctx->device = device_id;
	ctx->n_cus = prop.multiProcessorCount;
	if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
		delete ctx;
		return POLR_E_HIP;
	}
	*out = ctx;
	return POLR_OK;
}

void polr_ctx_destroy(polr_ctx *ctx) {
	POLR_ENTRY();
	if (!ctx) {
		return;
	}
	if (ctx->closed) {
		return; // (destroyed twice: the object only lives on for its children)
	}
	hipSetDevice(ctx->device);
	hipStreamSynchronize(ctx->stream);
	for (auto &f : ctx->pool_launches) {
		hipEventDestroy(f.done);
	}
	for (auto &e : ctx->pool_events_free) {
		hipEventDestroy(e);
	}
	ctx->pool_launches.clear();
	ctx->pool_events_free.clear();
	hipStreamDestroy(ctx->stream);
	// objects created on this context may outlive it (they hold references): what they still do -- free their
	// device memory -- needs the device ordinal only; the default stream stands in for the destroyed one
	ctx->stream = nullptr;
	ctx->closed = true;
	polr_ctx_release(ctx);
}

const char *polr_last_error(const polr_ctx *ctx) {
	return ctx ? ctx->err.c_str() : "no context (is a gfx950 device visible?)";
}

int polr_ctx_sync(polr_ctx *ctx, void *stream) {
	POLR_ENTRY();
	if (!ctx) {
		return POLR_E_INVALID;
	}
	HIPCHK(ctx, hipStreamSynchronize(polr_stream(ctx, stream)));
	return POLR_OK;
}

int polr_ctx_get_stream(polr_ctx *ctx, void **stream) {
	POLR_ENTRY();
	if (!ctx || !stream) {
		return POLR_E_INVALID;
	}
	*stream = (void *)ctx->stream;
	return POLR_OK;
}

int polr_ctx_set_pool_tuning(polr_ctx *ctx, const polr_pool_tuning *t) {
	POLR_ENTRY();
	if (!ctx) {
		return POLR_E_INVALID;
	}
	if (!t) {
		ctx->tuning = polr_pool_tuning {};
		return POLR_OK;
	}
	if (t->device_share > 16) {
		POLR_FAIL(ctx, POLR_E_INVALID, "device share 1/%u: at most 16 runs side by side", t->device_share);
	}
	if (t->units_x > 4) {
		POLR_FAIL(ctx, POLR_E_INVALID, "units_x %u: 1..4 (ring capacities are sized for 4)", t->units_x);
	}
	if (t->hi_unit && (t->hi_unit < 64 || t->hi_unit > 1024 || t->hi_unit % 64)) {
		POLR_FAIL(ctx, POLR_E_INVALID, "hi_unit %u: 64..1024 in multiples of 64", t->hi_unit);
	}
	if (t->hi_lottery & (t->hi_lottery - 1)) {
		POLR_FAIL(ctx, POLR_E_INVALID, "hi_lottery %u: a power of two", t->hi_lottery);
	}
	if (t->idle_sleep && t->idle_sleep != 16 && t->idle_sleep != 64) {
		POLR_FAIL(ctx, POLR_E_INVALID, "idle_sleep %u: 16 or 64", t->idle_sleep);
	}
	if (t->share_after && t->share_after != 0xFFFFFFFFu && (t->share_after < 16 || t->share_after > 65535)) {
		POLR_FAIL(ctx, POLR_E_INVALID, "share_after %u: 16..65535 steps, or 0xFFFFFFFF for never", t->share_after);
	}
	ctx->tuning = *t;
	return POLR_OK;
}

} // extern "C"

// ---------------------------------------------------------------------------------------------------
// helpers
// ---------------------------------------------------------------------------------------------------
// copy (or alias) a caller column to the device; acct: gains the bytes allocated
static int ingest_col(polr_ctx *ctx, const polr_col *src, uint64_t n_rows, OwnedCol *dst, uint64_t *acct,
                      hipStream_t st) {
	PolrBuildPlan plan;
	POLR_TRY_PLAN(ctx, plan, polr_build_check_col_width(src->width, plan));
	if (!src->data && n_rows) {
		POLR_FAIL(ctx, POLR_E_INVALID, "column data pointer is NULL");
	}
	dst->width = src->width;
	dst->flags = src->flags & POLR_COL_SIGNED;
	if (src->flags & POLR_COL_DEVICE) {
		dst->data = (uint8_t *)src->data;
		dst->valid = (uint8_t *)src->valid;
		return POLR_OK;
	}
	HIPCHK(ctx, dst->alloc_data(n_rows * src->width));
	*acct += dst->own_data.bytes();
	if (n_rows) {
		HIPCHK(ctx, hipMemcpyAsync(dst->data, src->data, n_rows * src->width, hipMemcpyHostToDevice, st));
	}
	if (src->valid) {
		HIPCHK(ctx, dst->alloc_valid(n_rows));
		*acct += dst->own_valid.bytes();
		if (n_rows) {
			HIPCHK(ctx, hipMemcpyAsync(dst->valid, src->valid, n_rows, hipMemcpyHostToDevice, st));
		}
	}
	return POLR_OK;
}

static int upload_devcols(polr_ctx *ctx, const std::vector<OwnedCol> &cols, DevBuf<DevCol> *dst, hipStream_t st) {
	std::vector<DevCol> h(cols.size() ? cols.size() : 1);
	for (size_t i = 0; i < cols.size(); i++) {
		h[i].data = cols[i].data;
		h[i].valid = cols[i].valid;
		h[i].width = cols[i].width;
		h[i].flags = cols[i].flags;
	}
	HIPCHK(ctx, dst->ensure(h.size()));
	HIPCHK(ctx, hipMemcpyAsync(dst->get(), h.data(), h.size() * sizeof(DevCol), hipMemcpyHostToDevice, st));
	HIPCHK(ctx, hipStreamSynchronize(st)); // h is a stack-lifetime staging buffer
	return POLR_OK;
}

// the last step of an upload: the key columns are a shape the kernels take, and their device array
static int accept_keys(polr_ht *ht) {
	polr_ctx *ctx = ht->ctx;
	std::vector<uint32_t> widths;
	for (auto &k : ht->keys) {
		widths.push_back(k.width);
	}
	PolrBuildPlan plan;
	POLR_TRY_PLAN(ctx, plan, polr_build_check_keys(widths.size(), widths.data(), plan));
	ht->key_signed = ht->keys[0].flags & POLR_COL_SIGNED;
	return upload_devcols(ctx, ht->keys, &ht->keys_dev, ctx->stream);
}

extern "C" {

// ---------------------------------------------------------------------------------------------------
// Build sides
// ---------------------------------------------------------------------------------------------------
int polr_ht_upload_columns(polr_ctx *ctx, const polr_col *keys, uint32_t n_keys, const polr_col *payload,
                           uint32_t n_payload, uint64_t n_rows, polr_ht **out) {
	POLR_ENTRY();
	if (!ctx || !out || !keys) {
		return POLR_E_INVALID;
	}
	*out = nullptr;
	PolrBuildPlan plan;
	POLR_TRY_PLAN(ctx, plan, polr_build_check_rows(n_rows, plan));
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HandleGuard<polr_ht> ht = polr_ht_new(ctx, n_keys, n_payload, n_rows);
	for (uint32_t i = 0; i < n_keys; i++) {
		POLR_TRY(ingest_col(ctx, &keys[i], n_rows, &ht->keys[i], &ht->device_bytes, ctx->stream));
	}
	for (uint32_t i = 0; i < n_payload; i++) {
		POLR_TRY(ingest_col(ctx, &payload[i], n_rows, &ht->payload[i], &ht->device_bytes, ctx->stream));
	}
	POLR_TRY(accept_keys(ht.get()));
	*out = ht.release();
	return POLR_OK;
}

int polr_ht_upload_rows(polr_ctx *ctx, const void *rows, uint64_t n_rows, uint32_t row_width,
                        const uint32_t *col_offset, const uint32_t *col_width, const uint32_t *col_flags,
                        uint32_t n_keys, uint32_t n_payload, polr_ht **out) {
	POLR_ENTRY();
	if (!ctx || !out || (!rows && n_rows) || !col_offset || !col_width) {
		return POLR_E_INVALID;
	}
	*out = nullptr;
	const uint32_t ncols = n_keys + n_payload;
	PolrBuildPlan plan;
	POLR_TRY_PLAN(ctx, plan, polr_build_check_rows(n_rows, plan));
	POLR_TRY_PLAN(ctx, plan, polr_build_check_row_layout(row_width, ncols, col_offset, col_width, plan));
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HandleGuard<polr_ht> ht = polr_ht_new(ctx, n_keys, n_payload, n_rows);
	DevBuf<uint8_t> blob;
	HIPCHK(ctx, blob.alloc(n_rows * row_width));
	if (n_rows) {
		HIPCHK(ctx, hipMemcpyAsync(blob, rows, n_rows * row_width, hipMemcpyHostToDevice, ctx->stream));
	}
	for (uint32_t c = 0; c < ncols; c++) {
		OwnedCol &col = c < n_keys ? ht->keys[c] : ht->payload[c - n_keys];
		col.width = col_width[c];
		col.flags = col_flags ? (col_flags[c] & POLR_COL_SIGNED) : 0;
		HIPCHK(ctx, col.alloc_data(n_rows * col.width));
		// (key columns too: a table whose condition is IS NOT DISTINCT FROM keeps its NULL-key rows, join_hashtable.cpp:182)
		HIPCHK(ctx, col.alloc_valid(n_rows));
		ht->device_bytes += col.own_data.bytes() + col.own_valid.bytes();
		polr_launch_deserialize_col(ctx->stream, blob, n_rows, row_width, c, col_offset[c], col.width, col.data,
		                            col.valid);
	}
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); // (the row de-serialisation; blob is a local)
	POLR_TRY(accept_keys(ht.get()));
	*out = ht.release();
	return POLR_OK;
}

int polr_ht_set_key_flags(polr_ht *ht, uint32_t key_col, uint32_t flags) {
	POLR_ENTRY();
	if (!ht) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = ht->ctx;
	if (ht->kind != KIND_NONE) {
		POLR_FAIL(ctx, POLR_E_INVALID, "key flags are set before the table is finalized");
	}
	if (key_col >= ht->n_keys || (flags & ~(POLR_KEY_BY_VALUE | POLR_KEY_NULL_EQUAL))) {
		POLR_FAIL(ctx, POLR_E_INVALID, "key column %u of %u, flags 0x%x", key_col, ht->n_keys, flags);
	}
	ht->key_flags[key_col] = flags;
	return POLR_OK;
}

int polr_ht_finalize_hash(polr_ht *ht, void *stream) {
	POLR_ENTRY();
	if (!ht) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = ht->ctx;
	if (ht->kind != KIND_NONE) {
		POLR_FAIL(ctx, POLR_E_INVALID, "table already finalized");
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	const uint64_t n = ht->n_rows_in;
	uint32_t key_width[POLR_MAX_KEYS] = {}, col_flags[POLR_MAX_KEYS] = {};
	for (uint32_t c = 0; c < ht->n_keys; c++) {
		key_width[c] = ht->keys[c].width;
		col_flags[c] = ht->keys[c].flags;
	}
	PolrKeyPackPlan packed; // (built here, stored with everything else once the build has succeeded)
	packed.pack = KeyPack();
	const KeyPack &pack = packed.pack;
	if (polr_build_needs_key_pack(ht->n_keys, key_width, ht->key_flags)) {
		// per-column [min, max] of the build keys (rows with a NULL key never match and do not count)
		long long h_mm[2 * POLR_NKEYS];
		for (uint32_t c = 0; c < POLR_NKEYS; c++) {
			h_mm[2 * c] = 0x7FFFFFFFFFFFFFFFll;
			h_mm[2 * c + 1] = -0x7FFFFFFFFFFFFFFFll - 1;
		}
		DevBuf<long long> mm;
		HIPCHK(ctx, mm.alloc(2 * POLR_NKEYS));
		HIPCHK(ctx, hipMemcpyAsync(mm, h_mm, sizeof(h_mm), hipMemcpyHostToDevice, st));
		const uint32_t null_eq = polr_build_null_eq_mask(ht->n_keys, ht->key_flags);
		polr_launch_key_minmax(st, ht->keys_dev, ht->n_keys, n, null_eq, mm);
		HIPCHK(ctx, hipMemcpyAsync(h_mm, mm, sizeof(h_mm), hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		POLR_TRY_PLAN(ctx, packed, polr_build_key_pack(ht->n_keys, h_mm, null_eq, col_flags, packed));
	}
	PolrCapacityPlan slots_plan;
	POLR_TRY_PLAN(ctx, slots_plan, polr_build_capacity(n, slots_plan));
	const uint64_t capacity = slots_plan.capacity;
	const uint64_t n_blocks = (capacity + 1023) / 1024;
	DevBuf<uint8_t> slots_mem; // [capacity] uint4: the table itself unless it is converted to 8-byte slots
	DevBuf<uint32_t> slot_of_row, cursor, rowids, block_sums, scalars;
	DevBuf<unsigned long long> n_valid;
	HIPCHK(ctx, slots_mem.alloc(capacity * sizeof(uint4)));
	HIPCHK(ctx, slot_of_row.alloc(n));
	HIPCHK(ctx, cursor.alloc(capacity));
	HIPCHK(ctx, rowids.alloc(n));
	HIPCHK(ctx, block_sums.alloc(n_blocks));
	HIPCHK(ctx, scalars.alloc(4));
	HIPCHK(ctx, n_valid.alloc(1));
	uint4 *slots = (uint4 *)slots_mem.get();
	uint32_t h_scalars[4] = {0, 0, 0, 0};
	unsigned long long h_valid = 0;
	HIPCHK(ctx, hipMemsetAsync(cursor, 0, capacity * 4, st));
	HIPCHK(ctx, hipMemsetAsync(scalars, 0, 16, st));
	HIPCHK(ctx, hipMemsetAsync(n_valid, 0, 8, st));
	polr_launch_s16_build(st, ht->keys_dev, ht->n_keys, pack, n, slots, capacity, slot_of_row, cursor, rowids, block_sums,
	                      scalars, n_valid);
	HIPCHK(ctx, hipMemcpyAsync(h_scalars, scalars, 16, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipMemcpyAsync(&h_valid, n_valid, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	// h_scalars: [0] sentinel rows, [1] longest run, [2] rows with a regular key
	polr_launch_s16_scatter(st, n, slots, slot_of_row, cursor, rowids, h_scalars[2], scalars + 3);
	HIPCHK(ctx, hipStreamSynchronize(st));
	PolrKindPlan kind;
	POLR_TRY_PLAN(ctx, kind, polr_build_hash_kind(h_scalars[1], h_scalars[0], ht->n_keys, key_width[0], pack.packed != 0, kind));
	const bool unique32 = kind.kind == KIND_S8;
	DevBuf<uint8_t> s8_mem; // [capacity] uint2
	if (unique32) {
		HIPCHK(ctx, s8_mem.alloc(capacity * sizeof(uint2)));
		polr_launch_s16_to_s8(st, slots, capacity, rowids, (uint2 *)s8_mem.get());
		HIPCHK(ctx, hipStreamSynchronize(st));
	}
	POLR_TRY(upload_devcols(ctx, ht->payload, &ht->payload_dev, st));
	// nothing can fail from here on: the table takes what was built
	ht->pack = pack;
	ht->n_rows = h_valid;
	ht->has_null = h_valid < n;
	ht->capacity = capacity;
	ht->sentinel_start = h_scalars[2];
	ht->sentinel_count = h_scalars[0];
	ht->max_run = kind.max_run;
	if (unique32) {
		ht->table_mem = std::move(s8_mem);
	} else {
		ht->table_mem = std::move(slots_mem);
		ht->rowids = std::move(rowids);
		ht->device_bytes += ht->rowids.bytes();
	}
	ht->device_bytes += ht->table_mem.bytes();
	ht->table = ht->table_mem;
	ht->kind = kind.kind;
	return POLR_OK;
}

// the re-ordered copies of the payload columns a perfect table of `size` slots reads; acct: gains the bytes allocated
static int alloc_perfect_cols(const polr_ht *ht, uint64_t size, std::vector<OwnedCol> &pcols, uint64_t *acct) {
	polr_ctx *ctx = ht->ctx;
	pcols.resize(ht->n_payload);
	for (uint32_t i = 0; i < ht->n_payload; i++) {
		OwnedCol &c = pcols[i];
		c.width = ht->payload[i].width;
		c.flags = ht->payload[i].flags;
		c.strings_rebased = ht->payload[i].strings_rebased; // (the re-ordered copy holds the same cells)
		HIPCHK(ctx, c.alloc_data(size * c.width));
		HIPCHK(ctx, c.alloc_valid(size));
		*acct += c.own_data.bytes() + c.own_valid.bytes();
	}
	return POLR_OK;
}

int polr_ht_finalize_perfect(polr_ht *ht, int64_t min_value, int64_t max_value, void *stream) {
	POLR_ENTRY();
	if (!ht) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = ht->ctx;
	if (ht->kind != KIND_NONE) {
		POLR_FAIL(ctx, POLR_E_INVALID, "table already finalized");
	}
	if (ht->n_keys != 1) {
		POLR_FAIL(ctx, POLR_E_UNSUPPORTED, "perfect hash join needs exactly one key (plan_comparison_join.cpp:63-133)");
	}
	if (ht->key_flags[0]) {
		POLR_FAIL(ctx, POLR_E_UNSUPPORTED, "a key compared by value (CAST) or with NULL = NULL takes a hash table "
		                                   "(the reference plans perfect hash joins for plain equalities only)");
	}
	const bool is_signed = ht->key_signed != 0;
	PolrPerfectPlan plan;
	POLR_TRY_PLAN(ctx, plan, polr_build_perfect_range(min_value, max_value, is_signed, plan));
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	const uint64_t range = plan.range, size = plan.size, words = plan.words;
	DevBuf<uint8_t> bits_mem; // [words] uint32_t
	DevBuf<uint32_t> idx_row, flags;
	DevBuf<unsigned long long> unique;
	HIPCHK(ctx, bits_mem.alloc(words * 4));
	HIPCHK(ctx, idx_row.alloc(size));
	HIPCHK(ctx, flags.alloc(2));
	HIPCHK(ctx, unique.alloc(1));
	uint32_t *bits = (uint32_t *)bits_mem.get();
	uint32_t h_flags[2] = {0, 0};
	unsigned long long h_unique = 0;
	HIPCHK(ctx, hipMemsetAsync(bits, 0, words * 4, st));
	HIPCHK(ctx, hipMemsetAsync(idx_row, 0xFF, size * 4, st));
	HIPCHK(ctx, hipMemsetAsync(flags, 0, 8, st));
	HIPCHK(ctx, hipMemsetAsync(unique, 0, 8, st));
	polr_launch_pht_mark(st, ht->keys_dev, ht->n_rows_in, min_value, range, is_signed ? 1 : 0, bits, idx_row, flags,
	                     unique);
	HIPCHK(ctx, hipMemcpyAsync(h_flags, flags, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipMemcpyAsync(&h_unique, unique, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	if (h_flags[0]) {
		POLR_FAIL(ctx, POLR_E_DUPLICATE, "duplicate build key inside the perfect-hash range");
	}
	std::vector<OwnedCol> pcols;
	uint64_t acct = bits_mem.bytes() + idx_row.bytes();
	POLR_TRY(alloc_perfect_cols(ht, size, pcols, &acct));
	for (uint32_t i = 0; i < ht->n_payload; i++) {
		polr_launch_pht_gather(st, bits, idx_row, size, dev_col(ht->payload[i]), pcols[i].data, pcols[i].valid);
	}
	HIPCHK(ctx, hipStreamSynchronize(st));
	POLR_TRY(upload_devcols(ctx, pcols, &ht->payload_dev, st));
	// nothing can fail from here on: the table takes what was built
	ht->table_mem = std::move(bits_mem);
	ht->idx_row = std::move(idx_row);
	ht->pcols = std::move(pcols);
	ht->device_bytes += acct;
	ht->min_value = min_value;
	ht->max_value = max_value;
	ht->range = range;
	ht->has_null = h_flags[1];
	ht->n_rows = h_unique;
	ht->capacity = size;
	ht->max_run = h_unique ? 1 : 0;
	ht->is_dense = (h_unique == size && !h_flags[1]) ? 1 : 0;
	ht->table = ht->bits = bits;
	ht->kind = KIND_PERFECT;
	return POLR_OK;
}

int polr_ht_finalize_auto(polr_ht *ht, int64_t min_value, int64_t max_value, void *stream, uint32_t *kind_out) {
	POLR_ENTRY();
	if (!ht) {
		return POLR_E_INVALID;
	}
	int rc = POLR_E_DUPLICATE;
	if (ht->kind == KIND_NONE &&
	    polr_build_auto_tries_perfect(ht->n_keys, ht->key_flags, ht->n_rows_in, min_value, max_value, ht->key_signed != 0)) {
		rc = polr_ht_finalize_perfect(ht, min_value, max_value, stream);
		if (rc != POLR_OK && rc != POLR_E_DUPLICATE) {
			return rc;
		}
	}
	if (rc == POLR_E_DUPLICATE) {
		rc = polr_ht_finalize_hash(ht, stream);
	}
	if (!rc && kind_out) {
		*kind_out = ht->kind;
	}
	return rc;
}

int polr_pht_upload(polr_ctx *ctx, uint32_t key_width, uint32_t key_flags, int64_t min_value, int64_t max_value,
                    const uint8_t *bitmap, const polr_col *payload, uint32_t n_payload, polr_ht **out) {
	POLR_ENTRY();
	if (!ctx || !out || !bitmap) {
		return POLR_E_INVALID;
	}
	*out = nullptr;
	const bool is_signed = (key_flags & POLR_COL_SIGNED) != 0;
	PolrPerfectPlan plan;
	POLR_TRY_PLAN(ctx, plan, polr_build_pht_upload(key_width, min_value, max_value, is_signed, plan));
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const uint64_t range = plan.range, size = plan.size;
	HandleGuard<polr_ht> ht = polr_ht_new(ctx, 1, n_payload, 0); // (n_rows_in: the bits set, counted below)
	ht->key_signed = is_signed ? POLR_COL_SIGNED : 0;
	ht->keys[0].width = key_width;
	ht->keys[0].flags = ht->key_signed;
	ht->pcols.resize(n_payload);
	for (uint32_t i = 0; i < n_payload; i++) {
		POLR_TRY(ingest_col(ctx, &payload[i], size, &ht->pcols[i], &ht->device_bytes, ctx->stream));
		ht->payload[i].width = ht->pcols[i].width;
	}
	DevBuf<uint8_t> bytes;
	HIPCHK(ctx, bytes.alloc(size));
	HIPCHK(ctx, ht->table_mem.alloc(plan.words * 4));
	ht->device_bytes += ht->table_mem.bytes();
	ht->bits = (uint32_t *)ht->table_mem.get();
	HIPCHK(ctx, hipMemcpyAsync(bytes, bitmap, size, hipMemcpyHostToDevice, ctx->stream));
	polr_launch_pack_bitmap(ctx->stream, bytes, size, ht->bits);
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	uint64_t set = 0;
	for (uint64_t i = 0; i < size; i++) {
		set += bitmap[i] ? 1 : 0;
	}
	ht->n_rows = ht->n_rows_in = set;
	ht->min_value = min_value;
	ht->max_value = max_value;
	ht->range = range;
	ht->capacity = size;
	ht->max_run = set ? 1 : 0;
	ht->is_dense = set == size;
	ht->table = ht->bits;
	ht->kind = KIND_PERFECT;
	POLR_TRY(upload_devcols(ctx, ht->pcols, &ht->payload_dev, ctx->stream));
	*out = ht.release();
	return POLR_OK;
}

void polr_ht_destroy(polr_ht *ht) {
	POLR_ENTRY();
	if (!ht) {
		return;
	}
	hipSetDevice(ht->ctx->device);
	polr_ctx *ctx_ = ht->ctx;
	delete ht;
	polr_ctx_release(ctx_);
}

int polr_ht_get_info(const polr_ht *ht, polr_ht_info *info) {
	POLR_ENTRY();
	if (!ht || !info) {
		return POLR_E_INVALID;
	}
	info->kind = ht->kind;
	info->n_keys = ht->n_keys;
	info->n_rows = ht->n_rows;
	info->capacity = ht->capacity;
	info->max_run = ht->max_run;
	info->device_bytes = ht->device_bytes;
	info->is_dense = ht->is_dense;
	info->has_null = ht->has_null;
	return POLR_OK;
}

// ---- export / alloc_like: the buffers a build-side broadcast has to move --------------------------
// (PolrHtMeta: polr_build_plan.h, with the list of buffers it implies and the check of a received one)
static void meta_buffers(const PolrHtMeta &m,std::vector<PolrBuildBuffer> &bufs) {
	polr_build_buffers(m.kind, m.capacity, m.n_rows_in, m.n_payload, m.payload_width, m.payload_has_valid, bufs);
}

static void fill_meta(const polr_ht *ht, PolrHtMeta &m) {
	memset(&m, 0, sizeof(m));
	m.magic = POLR_BUILD_META_MAGIC;
	m.kind = ht->kind;
	m.n_keys = ht->n_keys;
	m.n_payload = ht->n_payload;
	m.key_signed = ht->key_signed;
	m.is_dense = ht->is_dense;
	m.has_null = ht->has_null;
	m.sentinel_start = ht->sentinel_start;
	m.sentinel_count = ht->sentinel_count;
	m.n_rows_in = ht->n_rows_in;
	m.n_rows = ht->n_rows;
	m.capacity = ht->capacity;
	m.max_run = ht->max_run;
	m.range = ht->range;
	m.min_value = ht->min_value;
	m.max_value = ht->max_value;
	for (uint32_t i = 0; i < ht->n_keys; i++) {
		m.key_width[i] = ht->keys[i].width;
		m.key_flags[i] = ht->keys[i].flags;
		m.key_sem[i] = ht->key_flags[i];
	}
	m.pack = ht->pack;
	for (uint32_t i = 0; i < ht->n_payload; i++) {
		const OwnedCol &c = build_col(ht, i);
		m.payload_width[i] = c.width;
		m.payload_flags[i] = c.flags;
		m.payload_has_valid[i] = c.valid ? 1 : 0;
	}
}

// where the table keeps a buffer of the plan's list
static void *ht_buffer(const polr_ht *ht, const PolrBuildBuffer &b) {
	switch (b.what) {
	case POLR_BUF_TABLE:
		return ht->table;
	case POLR_BUF_ROWIDS:
		return ht->rowids;
	case POLR_BUF_COL_DATA:
		return build_col(ht, b.col).data;
	default:
		return build_col(ht, b.col).valid;
	}
}

int polr_ht_export(const polr_ht *ht, void *meta, uint64_t *meta_bytes, void **dev_ptrs, uint64_t *dev_bytes,
                   uint32_t *n_buffers) {
	POLR_ENTRY();
	if (!ht || !meta_bytes || !n_buffers) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = ht->ctx;
	if (ht->kind == KIND_NONE) {
		POLR_FAIL(ctx, POLR_E_INVALID, "table not finalized");
	}
	if (ht->n_payload > POLR_BUILD_MAX_PAYLOAD) {
		POLR_FAIL(ctx, POLR_E_UNSUPPORTED, "more than %u payload columns", POLR_BUILD_MAX_PAYLOAD);
	}
	PolrHtMeta m;
	fill_meta(ht, m);
	std::vector<PolrBuildBuffer> bufs;
	meta_buffers(m, bufs);
	const uint32_t cap_buffers = *n_buffers;
	const uint64_t cap_meta = *meta_bytes;
	*n_buffers = (uint32_t)bufs.size();
	*meta_bytes = sizeof(PolrHtMeta);
	if (!meta || !dev_ptrs || !dev_bytes) {
		return POLR_OK; // size query
	}
	if (cap_buffers < bufs.size() || cap_meta < sizeof(PolrHtMeta)) {
		POLR_FAIL(ctx, POLR_E_INVALID, "export buffers too small");
	}
	memcpy(meta, &m, sizeof(m));
	for (size_t i = 0; i < bufs.size(); i++) {
		dev_ptrs[i] = ht_buffer(ht, bufs[i]);
		dev_bytes[i] = bufs[i].bytes;
	}
	return POLR_OK;
}

int polr_ht_alloc_like(polr_ctx *ctx, const void *meta, uint64_t meta_bytes, polr_ht **out) {
	POLR_ENTRY();
	if (!ctx || !meta || !out || meta_bytes < sizeof(PolrHtMeta)) {
		return POLR_E_INVALID;
	}
	*out = nullptr;
	PolrHtMeta m;
	memcpy(&m, meta, sizeof(m));
	PolrBuildPlan plan;
	POLR_TRY_PLAN(ctx, plan, polr_build_check_meta(m, plan));
	std::vector<PolrBuildBuffer> bufs;
	meta_buffers(m, bufs);
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HandleGuard<polr_ht> ht = polr_ht_new(ctx, m.n_keys, m.n_payload, m.n_rows_in);
	ht->kind = m.kind;
	ht->key_signed = m.key_signed;
	ht->is_dense = m.is_dense;
	ht->has_null = m.has_null;
	ht->sentinel_start = m.sentinel_start;
	ht->sentinel_count = m.sentinel_count;
	ht->n_rows = m.n_rows;
	ht->capacity = m.capacity;
	ht->max_run = m.max_run;
	ht->range = m.range;
	ht->min_value = m.min_value;
	ht->max_value = m.max_value;
	for (uint32_t i = 0; i < m.n_keys; i++) {
		ht->keys[i].width = m.key_width[i];
		ht->keys[i].flags = m.n_keys == 1 ? m.key_signed : m.key_flags[i];
		ht->key_flags[i] = m.key_sem[i];
	}
	ht->pack = m.pack;
	std::vector<OwnedCol> &cols = m.kind == KIND_PERFECT ? ht->pcols : ht->payload;
	cols.resize(m.n_payload);
	for (uint32_t i = 0; i < m.n_payload; i++) {
		cols[i].width = ht->payload[i].width = m.payload_width[i];
		cols[i].flags = m.payload_flags[i];
	}
	// the buffers the sending side listed, each with the bytes it listed
	for (const PolrBuildBuffer &b : bufs) {
		switch (b.what) {
		case POLR_BUF_TABLE:
			HIPCHK(ctx, ht->table_mem.alloc(b.bytes));
			ht->table = ht->table_mem;
			ht->bits = m.kind == KIND_PERFECT ? (uint32_t *)ht->table_mem.get() : nullptr;
			break;
		case POLR_BUF_ROWIDS:
			HIPCHK(ctx, ht->rowids.alloc(m.n_rows_in));
			break;
		case POLR_BUF_COL_DATA:
			HIPCHK(ctx, cols[b.col].alloc_data(b.bytes));
			break;
		default:
			HIPCHK(ctx, cols[b.col].alloc_valid(b.bytes));
			break;
		}
		ht->device_bytes += b.bytes;
	}
	POLR_TRY(upload_devcols(ctx, cols, &ht->payload_dev, ctx->stream));
	*out = ht.release();
	return POLR_OK;
}

// ---------------------------------------------------------------------------------------------------
// Pipeline
// ---------------------------------------------------------------------------------------------------
static void fill_dev_join(DevJoin *dj, const polr_join_desc *jd, const polr_ht *ht) {
	memset(dj, 0, sizeof(*dj));
	dj->kind = ht->kind;
	dj->n_keys = ht->n_keys;
	for (uint32_t c = 0; c < ht->n_keys; c++) {
		dj->key_width[c] = ht->keys[c].width;
		dj->key_src_join[c] = jd->key_src_join[c];
		dj->key_src_col[c] = jd->key_src_col[c];
	}
	dj->key_signed = ht->key_signed ? 1 : 0;
	dj->n_payload = ht->n_payload;
	dj->mask = ht_mask(ht);
	dj->min_value = ht->min_value;
	dj->range = ht->range;
	dj->table = ht->table;
	dj->rowids = ht->rowids;
	dj->sentinel_start = ht->sentinel_start;
	dj->sentinel_count = ht->sentinel_count;
	dj->payload = ht->payload_dev;
	dj->n_preds = jd->n_preds;
	for (uint32_t c = 0; c < jd->n_preds && c < POLR_NPREDS; c++) {
		dj->pred_op[c] = jd->pred_op[c];
		dj->pred_src_join[c] = jd->pred_src_join[c];
		dj->pred_src_col[c] = jd->pred_src_col[c];
		dj->pred_build_col[c] = jd->pred_build_col[c];
	}
}

// one join as the plan sees it (polr_pipeline_plan.h): the caller's descriptor and what its build side is like
static PipePlanJoin plan_join(const polr_join_desc &jd) {
	PipePlanJoin t = PipePlanJoin();
	t.desc = jd;
	const polr_ht *ht = jd.ht;
	if (!ht || ht->kind == KIND_NONE) {
		return t; // (KIND_NONE: refused as not finalized)
	}
	t.kind = ht->kind;
	t.n_keys = ht->n_keys;
	for (uint32_t c = 0; c < ht->n_keys && c < POLR_NKEYS; c++) {
		t.key_width[c] = ht->keys[c].width;
		t.key_flags[c] = ht->key_flags[c];
	}
	t.key_signed = ht->key_signed ? 1 : 0;
	t.cols.reserve(ht->n_payload);
	for (uint32_t i = 0; i < ht->n_payload; i++) {
		const OwnedCol &col = build_col(ht, i);
		t.cols.push_back(PipeCol {col.width, col.flags & 1u});
	}
	t.capacity = ht->capacity;
	t.max_run = ht->max_run;
	t.min_value = ht->min_value;
	t.max_value = ht->max_value;
	t.range = ht->range;
	t.packed = ht->pack.packed;
	t.device = ht->ctx->device;
	t.table = ht->table;
	return t;
}

// the joins and join orders of a request as the plan sees them: everything of a PipePlanInput but the probe side
// (polr_pipeline_create below; polr_pipeline_from_output, polr_pipesrc.hip)
void polr_pipeline_plan_joins(polr_ctx *ctx, const polr_join_desc *joins, uint32_t k, const int32_t *paths, uint32_t n_paths,
                              PipePlanInput &in) {
	in.joins.clear();
	in.joins.reserve(k <= POLR_MAX_JOINS ? k : 0);
	in.device = ctx->device;
	in.k = k;
	in.n_paths = n_paths;
	for (uint32_t j = 0; j < k && k <= POLR_MAX_JOINS; j++) { // (any other k is refused before a join is looked at)
		in.joins.push_back(plan_join(joins[j]));
	}
	in.paths = paths;
	in.flat_wave_bytes = polr_pool_flat_wave_bytes(k);
}

// resolve every (join order, position) of a pipeline variant into a StageDesc (see polr_device.h)
// ext: extension records of the stages that need one (appended; StageDesc::ext holds the INDEX + 1 until the records
// have their device address, see polr_pipeline_create)
static void build_stage_descs(const polr_pipeline *p, const PipePlanInput &in, const PipePlan &plan, bool counting,
                              std::vector<StageDesc> &out, std::vector<StageExt> &ext) {
	const PipeSlots &slots = counting ? plan.count : plan.mat;
	out.assign((size_t)in.n_paths * POLR_KMAX, StageDesc());
	// the column a key or the left side of a condition is read from, and the tuple slot that holds its row
	auto source = [&](const PipeSource &s, int32_t &slot, const uint8_t *&data, const uint8_t *&valid) {
		const OwnedCol &col = s.join < 0 ? p->probe_cols[s.col] : build_col(p->hts[s.join], s.col);
		slot = s.join < 0 ? 0 : slots.slot_of_join[s.join];
		data = col.data;
		valid = col.valid;
	};
	for (uint32_t q = 0; q < in.n_paths; q++) {
		for (uint32_t pos = 0; pos < in.k; pos++) {
			const uint32_t j = (uint32_t)in.paths[q * in.k + pos];
			const polr_ht *ht = p->hts[j];
			const polr_join_desc &jd = in.joins[j].desc;
			const PipePlan::Join &pj = plan.joins[j];
			StageDesc &d = out[(size_t)q * POLR_KMAX + pos];
			memset(&d, 0, sizeof(d));
			d.kind = ht->kind;
			d.n_keys = ht->n_keys;
			d.key_signed = ht->key_signed ? 1 : 0;
			d.out_slot = slots.slot_of_join[j];
			for (uint32_t c = 0; c < ht->n_keys && c < 2; c++) {
				d.key_width[c] = ht->keys[c].width;
				source(pj.key[c], d.key_slot[c], d.key_data[c], d.key_valid[c]);
			}
			d.packed = ht->pack.packed;
			d.n_preds = jd.n_preds;
			if (pj.ext) {
				StageExt x;
				memset(&x, 0, sizeof(x));
				for (uint32_t c = 0; c < ht->n_keys; c++) {
					// width and signedness of the column a key is READ from (a key compared by value may differ from the build column)
					x.key_width[c] = pj.key[c].width;
					x.key_sx[c] = pj.key[c].sx;
					source(pj.key[c], x.key_slot[c], x.key_data[c], x.key_valid[c]);
				}
				x.pack = ht->pack;
				x.n_preds = jd.n_preds;
				for (uint32_t c = 0; c < jd.n_preds; c++) {
					const OwnedCol &bcol = build_col(ht, jd.pred_build_col[c]);
					x.pred_op[c] = jd.pred_op[c];
					x.pred_width[c] = bcol.width;
					x.pred_sx[c] = (bcol.flags & 1u) ? 1u : 0u;
					x.pred_bdata[c] = bcol.data;
					x.pred_bvalid[c] = bcol.valid;
					source(pj.pred[c], x.pred_slot[c], x.pred_data[c], x.pred_valid[c]);
				}
				ext.push_back(x);
				d.ext = (const StageExt *)(uintptr_t)ext.size(); // index + 1, patched to the device address later
			}
			d.table = ht->table;
			d.rowids = ht->rowids;
			d.mask = ht_mask(ht);
			d.min_value = ht->min_value;
			d.range = ht->range;
			d.sentinel_start = ht->sentinel_start;
			d.sentinel_count = ht->sentinel_count;
			d.unique = pj.unique;
			d.lds_off1 = counting ? pj.lds_off1 : 0u; // (only the counting variant runs on the flat kernel)
		}
	}
}

// one variant's header: which slot of a tuple carries which join's build id
static void set_slots(DevPipeline &dp, const PipeSlots &slots, uint32_t materialize, uint32_t mult) {
	dp.materialize = materialize;
	dp.W = slots.W;
	dp.mult = mult;
	for (uint32_t j = 0; j < POLR_KMAX; j++) {
		dp.slot_of_join[j] = slots.slot_of_join[j];
	}
}

// The rules -- what is refused, tuple slots, multiplicities, the flat kernel and its LDS tables -- are
// polr_pipeline_plan(); here the handles are described to it and its answer is written into the device structs.
int polr_pipeline_create(polr_ctx *ctx, const polr_col *probe_cols, uint32_t n_probe_cols, uint64_t n_probe_rows,
                         const polr_join_desc *joins, uint32_t k, const int32_t *paths, uint32_t n_paths,
                         polr_pipeline **out) {
	POLR_ENTRY();
	if (!ctx || !out || !joins || !paths || (!probe_cols && n_probe_cols)) {
		return POLR_E_INVALID;
	}
	*out = nullptr;
	PipePlanInput in;
	in.probe_cols.reserve(n_probe_cols);
	for (uint32_t i = 0; i < n_probe_cols; i++) {
		in.probe_cols.push_back(PipeCol {probe_cols[i].width, probe_cols[i].flags & POLR_COL_SIGNED});
	}
	in.n_probe_rows = n_probe_rows;
	polr_pipeline_plan_joins(ctx, joins, k, paths, n_paths, in);
	PipePlan plan;
	if (polr_pipeline_plan(in, plan)) {
		POLR_FAIL(ctx, plan.code, "%s", plan.msg);
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HandleGuard<polr_pipeline> guard(new polr_pipeline());
	polr_pipeline *p = guard.get();
	p->ctx = polr_ctx_retain(ctx);
	p->k = k;
	p->n_paths = n_paths;
	p->n_probe_cols = n_probe_cols;
	p->n_probe_rows = n_probe_rows;
	p->n_tuples = n_probe_rows;
	p->probe_cols.resize(n_probe_cols);
	uint64_t acct = 0;
	for (uint32_t i = 0; i < n_probe_cols; i++) {
		POLR_TRY(ingest_col(ctx, &probe_cols[i], n_probe_rows, &p->probe_cols[i], &acct, ctx->stream));
	}
	POLR_TRY(upload_devcols(ctx, p->probe_cols, &p->probe_cols_dev, ctx->stream));
	DevPipeline &m = p->host_mat, &c = p->host_count;
	memset(&m, 0, sizeof(m));
	m.k = k;
	m.n_paths = n_paths;
	m.n_probe_cols = n_probe_cols;
	m.probe_cols = p->probe_cols_dev;
	m.sel = nullptr;
	m.n_tuples = n_probe_rows;
	for (uint32_t j = 0; j < k; j++) {
		p->hts.push_back(joins[j].ht);
		fill_dev_join(&m.joins[j], &joins[j], joins[j].ht);
	}
	for (uint32_t q = 0; q < n_paths; q++) {
		for (uint32_t j = 0; j < k; j++) {
			m.paths[q].order[j] = (uint32_t)paths[q * k + j];
		}
	}
	c = m;
	set_slots(m, plan.mat, 1, 0);
	set_slots(c, plan.count, 0, plan.mult);
	c.flat = plan.flat;
	c.n_lds_tables = plan.n_lds_tables;
	c.lds_table_dwords = plan.lds_table_dwords;
	for (uint32_t t = 0; t < plan.n_lds_tables; t++) {
		c.lds_table_src[t] = (const uint32_t *)p->hts[plan.lds_table_join[t]]->table;
		c.lds_table_off[t] = plan.lds_table_off[t];
		c.lds_table_len[t] = plan.lds_table_len[t];
	}
	p->flat_wpb = plan.flat_wpb;
	p->flat_emit = plan.flat_emit != 0;
	std::vector<StageDesc> sd_mat, sd_count;
	std::vector<StageExt> sd_ext;
	build_stage_descs(p, in, plan, false, sd_mat, sd_ext);
	build_stage_descs(p, in, plan, true, sd_count, sd_ext);
	m.ext = c.ext = sd_ext.empty() ? 0u : 1u;
	if (!sd_ext.empty()) {
		HIPCHK(ctx, p->stage_ext.alloc(sd_ext.size()));
		HIPCHK(ctx, hipMemcpy(p->stage_ext, sd_ext.data(), sd_ext.size() * sizeof(StageExt), hipMemcpyHostToDevice));
		for (auto *sd : {&sd_mat, &sd_count}) {
			for (auto &d : *sd) {
				if (d.ext) {
					d.ext = p->stage_ext + ((uintptr_t)d.ext - 1);
				}
			}
		}
	}
	HIPCHK(ctx, p->stages_mat.alloc(sd_mat.size()));
	HIPCHK(ctx, p->stages_count.alloc(sd_count.size()));
	HIPCHK(ctx, hipMemcpy(p->stages_mat, sd_mat.data(), sd_mat.size() * sizeof(StageDesc), hipMemcpyHostToDevice));
	HIPCHK(ctx, hipMemcpy(p->stages_count, sd_count.data(), sd_count.size() * sizeof(StageDesc), hipMemcpyHostToDevice));
	m.stages = p->stages_mat;
	c.stages = p->stages_count;
	if (plan.flat) {
		// the counting variant's stages once more, in the flat kernel's own form (positions >= k stay zero: inert stages)
		std::vector<FlatStageRec> fs((size_t)n_paths * POLR_KMAX);
		memset(fs.data(), 0, fs.size() * sizeof(FlatStageRec));
		for (uint32_t q = 0; q < n_paths; q++) {
			for (uint32_t pos = 0; pos < k; pos++) {
				fs[(size_t)q * POLR_KMAX + pos] = flat_stage_rec(sd_count[(size_t)q * POLR_KMAX + pos], (uint32_t)paths[q * k + pos]);
			}
		}
		HIPCHK(ctx, p->stages_flat.alloc(fs.size()));
		HIPCHK(ctx, hipMemcpy(p->stages_flat, fs.data(), fs.size() * sizeof(FlatStageRec), hipMemcpyHostToDevice));
		c.flat_stages = p->stages_flat;
	}
	HIPCHK(ctx, p->dev_mat.alloc(1));
	HIPCHK(ctx, p->dev_count.alloc(1));
	HIPCHK(ctx, hipMemcpy(p->dev_mat, &m, sizeof(DevPipeline), hipMemcpyHostToDevice));
	HIPCHK(ctx, hipMemcpy(p->dev_count, &c, sizeof(DevPipeline), hipMemcpyHostToDevice));
	*out = guard.release();
	return POLR_OK;
}

int polr_pipeline_set_selection(polr_pipeline *p, const uint32_t *sel, uint64_t n_sel, uint32_t flags) {
	POLR_ENTRY();
	if (!p) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = p->ctx;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	p->sel_upload.reset();
	p->sel_dev = nullptr;
	p->scan_n_chunks = 0; // a caller-given selection replaces a scan result (its buffers stay for the next scan)
	p->scan_valid = false;
	if (!sel) {
		p->n_tuples = p->n_probe_rows;
	} else {
		if (flags & POLR_COL_DEVICE) {
			p->sel_dev = (uint32_t *)sel;
		} else {
			HIPCHK(ctx, p->sel_upload.alloc(n_sel));
			p->sel_dev = p->sel_upload;
			if (n_sel) {
				HIPCHK(ctx, hipMemcpy(p->sel_dev, sel, n_sel * 4, hipMemcpyHostToDevice));
			}
		}
		p->n_tuples = n_sel;
	}
	p->host_mat.sel = p->sel_dev;
	p->host_mat.n_tuples = p->n_tuples;
	p->host_count.sel = p->sel_dev;
	p->host_count.n_tuples = p->n_tuples;
	HIPCHK(ctx, hipMemcpy(p->dev_mat, &p->host_mat, sizeof(DevPipeline), hipMemcpyHostToDevice));
	HIPCHK(ctx, hipMemcpy(p->dev_count, &p->host_count, sizeof(DevPipeline), hipMemcpyHostToDevice));
	return POLR_OK;
}

int polr_pipeline_update_probe(polr_pipeline *p, uint32_t col, const void *data, const uint8_t *valid,
                               uint64_t n_rows) {
	POLR_ENTRY();
	if (!p || (!data && n_rows)) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = p->ctx;
	if (col >= p->n_probe_cols || n_rows > p->n_probe_rows) {
		POLR_FAIL(ctx, POLR_E_INVALID, "update of probe column %u with %llu rows does not fit (%u columns, %llu rows)",
		          col, (unsigned long long)n_rows, p->n_probe_cols, (unsigned long long)p->n_probe_rows);
	}
	OwnedCol &c = p->probe_cols[col];
	if (!c.owned()) {
		POLR_FAIL(ctx, POLR_E_INVALID, "probe column %u is caller-owned device memory", col);
	}
	if (valid && !c.valid) {
		POLR_FAIL(ctx, POLR_E_INVALID, "probe column %u was created without a validity array", col);
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (n_rows) {
		HIPCHK(ctx, hipMemcpyAsync(c.data, data, n_rows * c.width, hipMemcpyHostToDevice, ctx->stream));
		if (c.valid) {
			if (valid) {
				HIPCHK(ctx, hipMemcpyAsync(c.valid, valid, n_rows, hipMemcpyHostToDevice, ctx->stream));
			} else {
				HIPCHK(ctx, hipMemsetAsync(c.valid, 1, n_rows, ctx->stream));
			}
		}
	}
	if (!p->sel_dev) {
		p->n_tuples = n_rows;
		p->host_mat.n_tuples = n_rows;
		p->host_count.n_tuples = n_rows;
	}
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return POLR_OK;
}

void polr_pipeline_destroy(polr_pipeline *p) {
	POLR_ENTRY();
	if (!p) {
		return;
	}
	hipSetDevice(p->ctx->device);
	polr_ctx *ctx_ = p->ctx;
	delete p;
	polr_ctx_release(ctx_);
}

// ---------------------------------------------------------------------------------------------------
// Output chunks
// ---------------------------------------------------------------------------------------------------
int polr_out_create(polr_pipeline *p, uint32_t chunk_capacity, uint64_t max_chunks, polr_out **out) {
	POLR_ENTRY();
	if (!p || !out) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = p->ctx;
	*out = nullptr;
	if (chunk_capacity < 64 || chunk_capacity > 65536 || max_chunks < 1 || max_chunks > 0x7FFFFFFFull) {
		POLR_FAIL(ctx, POLR_E_INVALID, "output chunk capacity %u / max_chunks %llu out of range", chunk_capacity,
		          (unsigned long long)max_chunks);
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	HandleGuard<polr_out> o(new polr_out());
	o->pipe = p;
	o->ctx = polr_ctx_retain(p->ctx);
	memset(&o->dev, 0, sizeof(o->dev));
	o->dev.chunk_capacity = chunk_capacity;
	o->dev.max_chunks = (uint32_t)max_chunks;
	o->dev.W_out = 1 + p->k;
	o->dev.slot_stride = max_chunks * chunk_capacity;
	HIPCHK(ctx, o->ids.alloc(o->dev.slot_stride * o->dev.W_out));
	HIPCHK(ctx, o->chunk_count.alloc(max_chunks));
	HIPCHK(ctx, o->cursor.alloc(2));
	HIPCHK(ctx, o->chunk_base.alloc(max_chunks));
	HIPCHK(ctx, o->total_dev.alloc(1));
	o->dev.ids = o->ids;
	o->dev.chunk_count = o->chunk_count;
	o->dev.cursor = o->cursor;
	HIPCHK(ctx, hipMemset(o->dev.chunk_count, 0, max_chunks * 4));
	HIPCHK(ctx, hipMemset(o->dev.cursor, 0, 8));
	*out = o.release();
	return POLR_OK;
}

int polr_out_reset(polr_out *o, void *stream) {
	POLR_ENTRY();
	if (!o) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = o->pipe->ctx;
	hipStream_t st = polr_stream(ctx, stream);
	HIPCHK(ctx, hipMemsetAsync(o->dev.chunk_count, 0, (uint64_t)o->dev.max_chunks * 4, st));
	HIPCHK(ctx, hipMemsetAsync(o->dev.cursor, 0, 8, st));
	if (o->fused_cells) { // (a fused GROUP BY sink: its cells start from zero, too)
		HIPCHK(ctx, hipMemsetAsync(o->fused_cells, 0,
		                           (size_t)o->fused_tables * o->fused_groups * polr_fused_group_words(o->fused_aggs) * 8u, st));
		HIPCHK(ctx, hipMemsetAsync(o->fused_dropped, 0, 8, st));
	}
	if (o->agg_cells) { // (a fused ungrouped sink: its cells go back to "no rows" -- MIN's identity is not 0)
		polr_launch_fuseagg_fill(st, o);
	}
	// (runs that write this output on another stream wait for these memsets: out_order_behind_reset)
	if (!o->reset_event) {
		HIPCHK(ctx, hipEventCreateWithFlags(&o->reset_event, hipEventDisableTiming));
	}
	HIPCHK(ctx, hipEventRecord(o->reset_event, st));
	o->reset_stream = st;
	o->stats_valid = false;
	return POLR_OK;
}

int polr_out_stats(polr_out *o, void *stream, uint64_t *n_rows, uint64_t *n_chunks, uint32_t *overflowed) {
	POLR_ENTRY();
	if (!o) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = o->pipe->ctx;
	hipStream_t st = polr_stream(ctx, stream);
	uint32_t cur[2] = {0, 0};
	HIPCHK(ctx, hipMemcpyAsync(cur, o->dev.cursor, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	const uint32_t nc = std::min<uint32_t>(cur[0], o->dev.max_chunks);
	uint64_t total = 0;
	if (nc) {
		polr_launch_chunk_prefix(st, o->dev.chunk_count, nc, o->chunk_base, o->total_dev);
		HIPCHK(ctx, hipMemcpyAsync(&total, o->total_dev, 8, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
	}
	o->n_rows = total;
	o->n_chunks = nc;
	o->stats_valid = true;
	if (n_rows) {
		*n_rows = total;
	}
	if (n_chunks) {
		*n_chunks = nc;
	}
	if (overflowed) {
		*overflowed = cur[1];
	}
	return POLR_OK;
}

int polr_out_fetch_ids(polr_out *o, void *stream, uint32_t *dst, uint64_t dst_rows) {
	POLR_ENTRY();
	if (!o || (!dst && dst_rows)) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = o->pipe->ctx;
	POLR_REFUSE_AGG_CELLS(ctx, o);
	hipStream_t st = polr_stream(ctx, stream);
	int rc = out_ensure_stats(o, stream);
	if (rc) {
		return rc;
	}
	if (dst_rows < o->n_rows) {
		POLR_FAIL(ctx, POLR_E_INVALID, "destination holds %llu rows, output has %llu", (unsigned long long)dst_rows,
		          (unsigned long long)o->n_rows);
	}
	if (o->n_rows == 0) {
		return POLR_OK;
	}
	DevBuf<uint32_t> tmp;
	HIPCHK(ctx, tmp.alloc(o->n_rows * o->dev.W_out));
	polr_launch_compact_ids(st, o->dev, o->chunk_base, o->n_chunks, tmp);
	HIPCHK(ctx, hipMemcpyAsync(dst, tmp, o->n_rows * o->dev.W_out * 4, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	return POLR_OK;
}

int polr_out_materialize(polr_out *o, void *stream, int32_t src_join, uint32_t src_col, void *dst_data,
                         uint8_t *dst_valid, uint64_t dst_rows, uint32_t dst_flags) {
	POLR_ENTRY();
	if (!o || (!dst_data && dst_rows)) {
		return POLR_E_INVALID;
	}
	polr_pipeline *p = o->pipe;
	polr_ctx *ctx = p->ctx;
	POLR_REFUSE_AGG_CELLS(ctx, o);
	hipStream_t st = polr_stream(ctx, stream);
	int rc = out_ensure_stats(o, stream);
	if (rc) {
		return rc;
	}
	if (dst_rows < o->n_rows) {
		POLR_FAIL(ctx, POLR_E_INVALID, "destination holds %llu rows, output has %llu", (unsigned long long)dst_rows,
		          (unsigned long long)o->n_rows);
	}
	OutCol c;
	rc = polr_out_col(p, src_join, src_col, &c, "column", src_col);
	if (rc) {
		return rc;
	}
	const DevCol &src = c.dev;
	const uint32_t slot = c.slot;
	if (o->n_rows == 0) {
		return POLR_OK;
	}
	const bool to_device = (dst_flags & POLR_COL_DEVICE) != 0;
	uint8_t *d_data = (uint8_t *)dst_data, *d_valid = dst_valid;
	DevBuf<uint8_t> tmp_data, tmp_valid;
	if (!to_device) {
		HIPCHK(ctx, tmp_data.alloc(o->n_rows * src.width));
		d_data = tmp_data;
		if (dst_valid) {
			HIPCHK(ctx, tmp_valid.alloc(o->n_rows));
			d_valid = tmp_valid;
		}
	}
	polr_launch_gather(st, o->dev, o->chunk_base, o->n_chunks, slot, src, d_data, d_valid);
	if (!to_device) {
		HIPCHK(ctx, hipMemcpyAsync(dst_data, tmp_data, o->n_rows * src.width, hipMemcpyDeviceToHost, st));
		if (dst_valid) {
			HIPCHK(ctx, hipMemcpyAsync(dst_valid, tmp_valid, o->n_rows, hipMemcpyDeviceToHost, st));
		}
		HIPCHK(ctx, hipStreamSynchronize(st)); // (the temporaries are locals)
	}
	return POLR_OK;
}

void polr_out_destroy(polr_out *o) {
	POLR_ENTRY();
	if (!o) {
		return;
	}
	hipSetDevice(o->ctx->device);
	polr_ctx *ctx_ = o->ctx;
	if (o->reset_event) {
		hipEventDestroy(o->reset_event);
	}
	delete o;
	polr_ctx_release(ctx_);
}

} // extern "C"

// ---------------------------------------------------------------------------------------------------
// Probe launches
// ---------------------------------------------------------------------------------------------------
// Launch geometry: 256-thread workgroups (4 independent waves); the grid never exceeds what is
// resident at once (occupancy of the instantiation x CUs), waves grid-stride over units of 64..1024
// tuples sized so that a small routing round still spreads over the chip while a table-sized round
// gives every resident wave a few units.
uint32_t polr_waves_per_block(polr_pipeline *p, bool materialize) {
	const DevPipeline &dp = materialize ? p->host_mat : p->host_count;
	uint32_t &cached = materialize ? p->wpb_mat : p->wpb_count;
	if (cached == 0) {
		for (uint32_t w : {4u, 2u, 1u}) {
			// leave room for at least two workgroups per CU when possible
			if (polr_path_lds_bytes(dp.k, dp.W, w) <= (w == 1 ? 160u * 1024 : 80u * 1024)) {
				cached = w;
				break;
			}
		}
	}
	return cached;
}

uint32_t polr_resident_waves(polr_pipeline *p, bool materialize) {
	const DevPipeline &dp = materialize ? p->host_mat : p->host_count;
	const uint32_t wpb = polr_waves_per_block(p, materialize);
	int &cached = materialize ? p->blocks_per_cu_mat : p->blocks_per_cu_count;
	if (cached == 0) {
		cached = polr_path_occupancy(dp.k, dp.W, wpb);
		if (cached > 8) {
			cached = 8;
		}
	}
	return (uint32_t)p->ctx->n_cus * (uint32_t)cached * wpb;
}

int polr_plan_launch(polr_pipeline *p, bool materialize, uint64_t total_tuples, uint32_t *unit_size,
                     uint32_t *n_blocks_max) {
	const uint32_t wpb = polr_waves_per_block(p, materialize);
	if (wpb == 0) {
		p->ctx->err = "per-wave LDS queues exceed 160 KB (too many joins x carried ids)";
		return POLR_E_UNSUPPORTED;
	}
	const uint64_t waves = polr_resident_waves(p, materialize);
	uint64_t us = (total_tuples + waves - 1) / waves;
	us = ((us + 63) / 64) * 64;
	us = std::min<uint64_t>(std::max<uint64_t>(us, 64), 2048);
	*unit_size = (uint32_t)us;
	*n_blocks_max = (uint32_t)(waves / wpb);
	return POLR_OK;
}

extern "C" {

int polr_probe_rounds_async(polr_pipeline *p, void *stream, const polr_round *rounds, uint32_t n_rounds,
                            polr_out *out, uint64_t *counts_dev) {
	POLR_ENTRY();
	if (!p || !rounds || !counts_dev || n_rounds == 0) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = p->ctx;
	if (out && out->pipe != p) {
		POLR_FAIL(ctx, POLR_E_INVALID, "output object belongs to another pipeline");
	}
	POLR_REFUSE_FUSED(ctx, out);
	uint64_t total = 0;
	for (uint32_t r = 0; r < n_rounds; r++) {
		if (rounds[r].path >= p->n_paths) {
			POLR_FAIL(ctx, POLR_E_INVALID, "round %u: path %u out of range", r, rounds[r].path);
		}
		if (rounds[r].begin > p->n_tuples || rounds[r].count > p->n_tuples - rounds[r].begin) {
			POLR_FAIL(ctx, POLR_E_INVALID, "round %u: tuples [%llu, +%llu) outside the %llu tuples of the source", r,
			          (unsigned long long)rounds[r].begin, (unsigned long long)rounds[r].count,
			          (unsigned long long)p->n_tuples);
		}
		total += rounds[r].count;
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	if (total == 0) {
		HIPCHK(ctx, hipMemsetAsync(counts_dev, 0, (uint64_t)n_rounds * p->k * 8, st));
		return POLR_OK;
	}
	const uint64_t need_shards = (uint64_t)n_rounds * POLR_NSHARD * p->k;
	if (need_shards > p->shards_dev.size()) {
		if (p->shards_dev) {
			HIPCHK(ctx, hipStreamSynchronize(st)); // (the stream may still read what ensure frees)
		}
		HIPCHK(ctx, p->shards_dev.ensure(std::max<uint64_t>(need_shards, 64 * POLR_NSHARD * POLR_KMAX)));
	}
	HIPCHK(ctx, hipMemsetAsync(p->shards_dev, 0, need_shards * 8, st));
	const bool materialize = out != nullptr;
	uint32_t unit_size, max_blocks;
	int rc = polr_plan_launch(p, materialize, total, &unit_size, &max_blocks);
	if (rc) {
		return rc;
	}
	// (three buffers, each with its own capacity: a failed allocation leaves that one empty, and the next call grows it)
	if (n_rounds > p->rounds_dev.size() || n_rounds + 1 > p->prefix_dev.size() || n_rounds > p->unit_sizes_dev.size()) {
		if (p->rounds_dev || p->prefix_dev || p->unit_sizes_dev) {
			HIPCHK(ctx, hipStreamSynchronize(st));
		}
		const uint64_t cap = std::max<uint32_t>(n_rounds, 64);
		HIPCHK(ctx, p->rounds_dev.ensure(cap));
		HIPCHK(ctx, p->prefix_dev.ensure(cap + 1));
		HIPCHK(ctx, p->unit_sizes_dev.ensure(cap));
	}
	std::vector<uint64_t> prefix(n_rounds + 1);
	std::vector<uint32_t> usizes(n_rounds, unit_size);
	prefix[0] = 0;
	for (uint32_t r = 0; r < n_rounds; r++) {
		prefix[r + 1] = prefix[r] + (rounds[r].count + unit_size - 1) / unit_size;
	}
	static_assert(sizeof(DevRound) == sizeof(polr_round), "round layout");
	// pageable source: the runtime stages it before returning, so the caller's array may be reused
	HIPCHK(ctx, hipMemcpyAsync(p->rounds_dev, rounds, (uint64_t)n_rounds * sizeof(DevRound), hipMemcpyHostToDevice, st));
	HIPCHK(ctx, hipMemcpyAsync(p->prefix_dev, prefix.data(), ((uint64_t)n_rounds + 1) * 8, hipMemcpyHostToDevice, st));
	HIPCHK(ctx, hipMemcpyAsync(p->unit_sizes_dev, usizes.data(), (uint64_t)n_rounds * 4, hipMemcpyHostToDevice, st));
	HIPCHK(ctx, hipStreamSynchronize(st)); // prefix is a local vector
	const uint64_t total_units = prefix[n_rounds];
	const uint32_t wpb = polr_waves_per_block(p, materialize);
	const uint32_t n_blocks = (uint32_t)std::min<uint64_t>(max_blocks, (total_units + wpb - 1) / wpb);
	DevOut dout;
	memset(&dout, 0, sizeof(dout));
	if (out) {
		dout = out->dev;
		out->stats_valid = false;
		HIPCHK(ctx, out_order_behind_reset(out, st));
	}
	const DevPipeline &dp = materialize ? p->host_mat : p->host_count;
	hipError_t e = polr_launch_path_kernel(dp.W, dp.k, n_blocks, wpb, st, materialize ? p->dev_mat : p->dev_count,
	                                       p->rounds_dev, p->prefix_dev, n_rounds, p->unit_sizes_dev, dout,
	                                       p->shards_dev, SelfRoute {});
	if (e != hipSuccess) {
		POLR_FAIL(ctx, POLR_E_HIP, "path kernel launch failed: %s", hipGetErrorString(e));
	}
	polr_launch_reduce_counts(st, p->shards_dev, n_rounds, p->k, (unsigned long long *)counts_dev);
	return POLR_OK;
}

int polr_probe_rounds(polr_pipeline *p, void *stream, const polr_round *rounds, uint32_t n_rounds, polr_out *out,
                      uint64_t *counts) {
	POLR_ENTRY();
	if (!p || !counts) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = p->ctx;
	POLR_REFUSE_FUSED(ctx, out);
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	const uint64_t need = (uint64_t)n_rounds * p->k;
	if (need > p->counts_dev.size()) {
		HIPCHK(ctx, p->counts_dev.ensure(std::max<uint64_t>(need, 256)));
	}
	int rc = polr_probe_rounds_async(p, stream, rounds, n_rounds, out, (uint64_t *)p->counts_dev.get());
	if (rc) {
		return rc;
	}
	HIPCHK(ctx, hipMemcpyAsync(counts, p->counts_dev, need * 8, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	if (out) {
		uint32_t cur[2];
		HIPCHK(ctx, hipMemcpy(cur, out->dev.cursor, 8, hipMemcpyDeviceToHost));
		if (cur[1]) {
			POLR_FAIL(ctx, POLR_E_OVERFLOW, "output needs more than %u chunks of %u rows (counters are exact)",
			          out->dev.max_chunks, out->dev.chunk_capacity);
		}
	}
	return POLR_OK;
}

} // extern "C"
