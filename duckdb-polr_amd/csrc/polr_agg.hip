// duckdb-polr_amd/csrc/polr_agg.hip -- the sink side of the POLAR pipeline on the device.
//
// Reference: PhysicalUngroupedAggregate (src/execution/operator/aggregate/physical_ungrouped_aggregate.cpp)
// folds every chunk the pipeline produces into one state per aggregate: COUNT(*) counts rows
// (src/function/aggregate/distributive/count.cpp), COUNT(x) the non-NULL x, SUM(x) adds the non-NULL x exactly
// in a HUGEINT (sum.cpp:113-144 SumToHugeintOperation; NULL when nothing was added, sum_helpers.hpp isset),
// MIN / MAX keep the extreme of the non-NULL x (minmax.cpp; NULL when there was none).
//
// Here the pipeline's result is a stream of row-id chunks (polr_out); the aggregate never materialises a
// column: one pass gathers x by row id and reduces it -- thread-local, wave shuffle, one partial per
// workgroup -- and only the per-workgroup partials (a few KB) leave the device; the host adds them up in
// 128-bit arithmetic.  Algorithmic bytes: 4 (row id) + width [+ 1 validity] per output row and aggregate.
//
// What a sink refuses, in which order and with which words, is polr_agg_plan.h (host code without HIP): every sink here
// resolves the columns its request names, describes them to its plan, and builds its device structs from what the plan
// accepted.  Behind the plan a sink fails only for HIP errors and for what the device alone can tell: arguments out of
// range, too many groups, a string arena too small, a string column whose heap never came (polr_strheap.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "polr_internal.h"
#include "polr_strrec_plan.h" // the groups' strings leave as records (polr_fetch_str_records)

struct AggPartial {
	unsigned long long sum_lo; // two's complement 128-bit sum, low limb
	long long sum_hi;
	long long mn, mx;
	unsigned long long count; // rows that took part (non-NULL; all rows for COUNT(*))
};

// ---- aggregate ARGUMENTS that are `left OP right` (polr_out_aggregate*_expr): what the reference evaluates in the projection
// under its aggregate operators, with the checked operators of src/include/duckdb/common/operator/{add,subtract,multiply}.hpp
// (TryAddOperator / TrySubtractOperator / TryMultiplyOperator: the exact result must lie in the result type, else
// OutOfRangeException).  The expression form has a set of its own -- FusedSink embeds DevAgg / DevAggSet, whose layout
// stays -- and the sink kernels are compiled once per set type.  The set type decides how an argument is fetched (arg_value)
// and what tallies the arguments out of range (Oor): each kernel has one body, and the plain form pays for neither the
// operator dispatch nor the range compare.
struct DevExprAgg {
	DevCol src[2];    // left, right operand ([0] alone for POLR_ARG_COLUMN)
	uint32_t slot[2]; // the row ids that index them
	uint32_t fn, op;
	long long lo, hi; // the range of the declared result type
};
struct DevExprAggSet {
	DevExprAgg a[POLR_MAX_AGGS];
	uint32_t n;
	uint32_t pad;
	unsigned long long *oor; // [POLR_MAX_AGGS]: arguments out of range, added by every wave under the first aggregate IT saw one for
};

// a lane's count of out-of-range arguments and the lowest aggregate index it saw one for
struct OorCount {
	unsigned long long n = 0;
	uint32_t first = 0xFFFFFFFFu;
};
// ... and the plain form's: a column is never out of range
struct NoOor {};

template <class SET>
struct set_traits {
	static constexpr bool expr = false;
	using Oor = NoOor;
};
template <>
struct set_traits<DevExprAggSet> {
	static constexpr bool expr = true;
	using Oor = OorCount;
};

// The argument of aggregate `ag` for the output row at position `at` of every slot's row-id array: false = NULL (an operand is
// NULL: the row takes no part and cannot overflow) or out of range (counted; the call will fail and no result leaves).
// The plain form: the column's cell.
__device__ __forceinline__ bool arg_value(const DevOut &out, uint64_t at, const DevAgg &ag, uint32_t, long long *v, NoOor *) {
	const uint32_t row = out.ids[(uint64_t)ag.slot * out.slot_stride + at];
	if (ag.src.valid && !ag.src.valid[row]) {
		return false;
	}
	*v = load_col_cell(ag.src, row);
	return true;
}

// The expression form.  Operands are cells of at most 8 bytes, signed if 8, so both are exact in 64 bits and the overflow flag
// of the 64-bit operation plus the comparison with [lo, hi] is the reference's test for every result type up to BIGINT.
__device__ __forceinline__ bool arg_value(const DevOut &out, uint64_t at, const DevExprAgg &ag, uint32_t a, long long *v, OorCount *oor) {
	const uint32_t r0 = out.ids[(uint64_t)ag.slot[0] * out.slot_stride + at];
	if (ag.op == POLR_ARG_COLUMN) {
		if (ag.src[0].valid && !ag.src[0].valid[r0]) {
			return false;
		}
		*v = load_col_cell(ag.src[0], r0);
		return true;
	}
	// (both operands of one source: the row id is read once)
	const uint32_t r1 = ag.slot[1] == ag.slot[0] ? r0 : out.ids[(uint64_t)ag.slot[1] * out.slot_stride + at];
	if ((ag.src[0].valid && !ag.src[0].valid[r0]) || (ag.src[1].valid && !ag.src[1].valid[r1])) {
		return false;
	}
	const long long x = load_col_cell(ag.src[0], r0), y = load_col_cell(ag.src[1], r1);
	long long r;
	bool over;
	switch (ag.op) {
	case POLR_ARG_ADD:
		over = __builtin_add_overflow(x, y, &r);
		break;
	case POLR_ARG_SUB:
		over = __builtin_sub_overflow(x, y, &r);
		break;
	default:
		over = __builtin_mul_overflow(x, y, &r);
		break;
	}
	if (over || r < ag.lo || r > ag.hi) {
		oor->n++;
		oor->first = a < oor->first ? a : oor->first;
		return false;
	}
	*v = r;
	return true;
}

// once per wave, all lanes converged: one atomic, and none when the wave saw nothing out of range
__device__ __forceinline__ void flush_oor(const DevAggSet &, const NoOor &) {
}
__device__ __forceinline__ void flush_oor(const DevExprAggSet &aggs, const OorCount &mine) {
	unsigned long long *oor = aggs.oor;
	const unsigned long long n = wave_sum64(mine.n);
	if (n) {
		uint32_t first = mine.first;
#pragma unroll
		for (int d = 32; d > 0; d >>= 1) {
			const uint32_t o = (uint32_t)__shfl_xor((int)first, d, 64);
			first = o < first ? o : first;
		}
		if ((threadIdx.x & 63u) == 0) {
			atomicAdd(&oor[first], n);
		}
	}
}

// grid-stride over the output chunks; partials[blockIdx.x * n + a]
template <class SET>
__global__ __launch_bounds__(256) void polr_agg_kernel(DevOut out, uint32_t n_chunks, SET aggs,
                                                       AggPartial *__restrict__ partials) {
	typename set_traits<SET>::Oor my_oor;
	__shared__ AggPartial wave_part[4][POLR_MAX_AGGS];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (uint32_t a = 0; a < aggs.n; a++) {
		const auto ag = aggs.a[a];
		unsigned long long lo = 0, cnt = 0;
		long long hi = 0, mn = 0x7FFFFFFFFFFFFFFFll, mx = (long long)0x8000000000000000ull;
		for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
			const uint32_t n = out.chunk_count[chunk];
			const uint64_t chunk_base = (uint64_t)chunk * out.chunk_capacity;
			for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
				if (ag.fn == POLR_AGG_COUNT_STAR) {
					cnt++;
					continue;
				}
				long long v;
				if (!arg_value(out, chunk_base + i, ag, a, &v, &my_oor)) {
					continue; // NULLs take no part; nor does an argument out of range
				}
				cnt++;
				const unsigned long long nl = lo + (unsigned long long)v;
				hi += (v < 0 ? -1 : 0) + (nl < lo ? 1 : 0); // sign extension of v + carry
				lo = nl;
				mn = v < mn ? v : mn;
				mx = v > mx ? v : mx;
			}
		}
		// wave reduction (128-bit add with carry, min, max, count)
		for (int d = 32; d > 0; d >>= 1) {
			const unsigned long long olo = __shfl_down(lo, d, 64);
			const long long ohi = __shfl_down(hi, d, 64);
			const long long omn = __shfl_down(mn, d, 64), omx = __shfl_down(mx, d, 64);
			const unsigned long long ocnt = __shfl_down(cnt, d, 64);
			const unsigned long long nl = lo + olo;
			hi += ohi + (nl < lo ? 1 : 0);
			lo = nl;
			mn = omn < mn ? omn : mn;
			mx = omx > mx ? omx : mx;
			cnt += ocnt;
		}
		if (lane == 0) {
			wave_part[wave][a].sum_lo = lo;
			wave_part[wave][a].sum_hi = hi;
			wave_part[wave][a].mn = mn;
			wave_part[wave][a].mx = mx;
			wave_part[wave][a].count = cnt;
		}
	}
	flush_oor(aggs, my_oor);
	__syncthreads();
	if (threadIdx.x < aggs.n) {
		const uint32_t a = threadIdx.x;
		AggPartial r = wave_part[0][a];
		for (uint32_t w = 1; w < (blockDim.x >> 6); w++) {
			const AggPartial o = wave_part[w][a];
			const unsigned long long nl = r.sum_lo + o.sum_lo;
			r.sum_hi += o.sum_hi + (nl < r.sum_lo ? 1 : 0);
			r.sum_lo = nl;
			r.mn = o.mn < r.mn ? o.mn : r.mn;
			r.mx = o.mx > r.mx ? o.mx : r.mx;
			r.count += o.count;
		}
		partials[(uint64_t)blockIdx.x * aggs.n + a] = r;
	}
}

static_assert(POLR_MAX_AGGS == POLR_AGG_MAX_AGGS && POLR_MAX_GROUP_KEYS == POLR_AGG_MAX_GROUP_KEYS, "the sinks' plan: polr_agg_plan.h");

// a sink's plan (polr_agg_plan.h): its NULL-argument refusals carry no message and leave the context's error as it was
#define POLR_TRY_SINK_PLAN(ctx_, plan_, call_)                                                                         \
	do {                                                                                                               \
		const int sink_rc_ = (call_);                                                                                  \
		if (sink_rc_ && !(plan_).err[0]) {                                                                             \
			return sink_rc_;                                                                                           \
		}                                                                                                              \
		POLR_TRY_PLAN(ctx_, plan_, sink_rc_);                                                                          \
	} while (0)

PolrAggCol polr_out_describe_col(polr_pipeline *p, int32_t src_join, uint32_t src_col, OutCol *c) {
	PolrAggCol d = {false, 0, 0};
	if (src_join < 0 ? src_col >= p->n_probe_cols : ((uint32_t)src_join >= p->k || src_col >= p->hts[src_join]->n_payload)) {
		return d;
	}
	c->col = src_join < 0 ? &p->probe_cols[src_col] : &build_col(p->hts[src_join], src_col);
	c->slot = src_join < 0 ? 0 : 1 + (uint32_t)src_join;
	c->dev = dev_col(*c->col);
	d.in_range = true;
	d.width = c->dev.width;
	d.flags = c->dev.flags;
	return d;
}

int polr_out_col(polr_pipeline *p, int32_t src_join, uint32_t src_col, OutCol *c, const char *what, uint32_t idx) {
	if (!polr_out_describe_col(p, src_join, src_col, c).in_range) {
		char err[256];
		const int rc = polr_agg_col_out_of_range(src_join, src_col, what, idx, err);
		POLR_FAIL(p->ctx, rc, "%s", err);
	}
	return POLR_OK;
}

// The aggregates of one sink call, in the form the call was made in: the function codes polr_agg_decode / cell_value need and the
// device set of that form.  The entry point names the specs; the sink resolves their columns and describes them to its
// plan (describe_sink), and builds the device set from what the plan accepted (build_sink_aggs).
struct SinkAggs {
	SinkAggs(const polr_agg_spec *specs, uint32_t n_aggs) : n(n_aggs), expr(false), specs(specs) {
	}
	SinkAggs(const polr_agg_expr *specs, uint32_t n_aggs) : n(n_aggs), expr(true), specs(specs) {
	}
	uint32_t n;
	bool expr;
	const void *specs; // polr_agg_expr[n] if expr, else polr_agg_spec[n]
	uint32_t fn[POLR_MAX_AGGS];
	DevAggSet cols;      // !expr
	DevExprAggSet exprs; // expr
	PolrAggArg args[POLR_MAX_AGGS]; // as described to the plan
	OutCol src[POLR_MAX_AGGS][2];   // the operand columns, resolved where they are in range
};

// The head of every sink's request: the output, and the aggregates with their operand columns resolved and described.
// -> the context, or nullptr for a NULL output (which every plan refuses first, without a message)
static polr_ctx *describe_sink(polr_out *o, SinkAggs *s, PolrAggRequest *rq) {
	if (!o) {
		return nullptr;
	}
	rq->has_out = true;
	rq->agg_cells = o->agg_dev.get() != nullptr;
	rq->already_fused = out_has_fused_sink(o);
	rq->has_specs = s->specs != nullptr;
	rq->n_aggs = s->n;
	rq->args = s->args;
	for (uint32_t a = 0; s->specs && a < s->n && a < POLR_MAX_AGGS; a++) {
		PolrAggArg &g = s->args[a];
		g = s->expr ? polr_agg_arg_of(((const polr_agg_expr *)s->specs)[a]) : polr_agg_arg_of(((const polr_agg_spec *)s->specs)[a]);
		for (uint32_t x = 0; x < 2; x++) {
			g.col[x] = polr_out_describe_col(o->pipe, g.src_join[x], g.src_col[x], &s->src[a][x]);
		}
	}
	return o->pipe->ctx;
}

// ... and the device set of the call's form, from the plan that accepted them
static void build_sink_aggs(const PolrAggArgPlan *accepted, SinkAggs *s) {
	memset(&s->cols, 0, sizeof(s->cols));
	memset(&s->exprs, 0, sizeof(s->exprs));
	s->cols.n = s->exprs.n = s->n;
	for (uint32_t a = 0; a < s->n; a++) {
		const PolrAggArgPlan &ap = accepted[a];
		const uint32_t n_operands = polr_agg_n_operands(ap);
		const OutCol *c = s->src[a];
		DevExprAgg &e = s->exprs.a[a];
		s->fn[a] = s->cols.a[a].fn = e.fn = ap.fn;
		e.op = ap.op;
		e.lo = ap.lo;
		e.hi = ap.hi;
		for (uint32_t x = 0; x < 2 && n_operands; x++) { // (POLR_ARG_COLUMN: the one operand stands for both)
			e.src[x] = c[x < n_operands ? x : 0].dev;
			e.slot[x] = c[x < n_operands ? x : 0].slot;
		}
		if (n_operands) {
			s->cols.a[a].src = c[0].dev;
			s->cols.a[a].slot = c[0].slot;
		}
	}
}

// the group columns of a grouped sink's request, resolved and described
struct SinkGroups {
	PolrAggGroupCol cols[POLR_MAX_GROUP_KEYS];
	OutCol src[POLR_MAX_GROUP_KEYS];
};
static void describe_sink_groups(polr_out *o, const polr_group_key *keys, uint32_t n_keys, SinkGroups *g, PolrAggRequest *rq) {
	rq->has_keys = keys != nullptr;
	rq->n_keys = n_keys;
	rq->keys = g->cols;
	for (uint32_t q = 0; o && keys && q < n_keys && q < POLR_MAX_GROUP_KEYS; q++) {
		g->cols[q].src_join = keys[q].src_join;
		g->cols[q].src_col = keys[q].src_col;
		g->cols[q].n_values = keys[q].n_values;
		g->cols[q].col = polr_out_describe_col(o->pipe, keys[q].src_join, keys[q].src_col, &g->src[q]);
	}
}
// ... and as the sink kernels read them (domain: the perfect-hash sinks'; the hashed sink ignores it)
static DevGroupSet dev_group_set(const polr_group_key *keys, uint32_t n_keys, const SinkGroups &g, uint64_t n_groups) {
	DevGroupSet gs;
	memset(&gs, 0, sizeof(gs));
	gs.n = n_keys;
	gs.n_groups = (uint32_t)n_groups;
	for (uint32_t q = 0; q < n_keys; q++) {
		gs.k[q].src = g.src[q].dev;
		gs.k[q].slot = g.src[q].slot;
		gs.k[q].n_values = keys[q].n_values;
		gs.k[q].min_value = keys[q].min_value;
	}
	return gs;
}

// f(the device set of the call's form): where a sink's kernel is instantiated per set type
template <class F>
static void with_set(const SinkAggs &s, F &&f) {
	if (s.expr) {
		f(s.exprs);
	} else {
		f(s.cols);
	}
}

// A sink's counters on the device: `own` words of the sink's, and behind them -- the expression form only -- the out-of-range
// counters of its aggregates.
struct SinkCounters {
	static constexpr uint32_t MAX_OWN = 8;
	SinkCounters(const SinkAggs &aggs, uint32_t own) : own(own), n(own + (aggs.expr ? POLR_MAX_AGGS : 0)) {
	}
	size_t bytes() const {
		return (size_t)n * 8;
	}
	void place(unsigned long long *at, SinkAggs *aggs) {
		dev = at;
		aggs->exprs.oor = at + own;
	}
	hipError_t zero(hipStream_t st) {
		return n ? hipMemsetAsync(dev, 0, bytes(), st) : hipSuccess;
	}
	hipError_t fetch(hipStream_t st) {
		return n ? hipMemcpyAsync(host, dev, bytes(), hipMemcpyDeviceToHost, st) : hipSuccess;
	}
	// the arguments out of range of the call; first: the lowest aggregate that had one
	unsigned long long out_of_range(uint32_t *first = nullptr) const {
		unsigned long long total = 0;
		for (uint32_t a = POLR_MAX_AGGS; a-- > 0;) {
			total += host[own + a];
			if (host[own + a] && first) {
				*first = a;
			}
		}
		return total;
	}
	// the counters as the kernels left them -> POLR_E_RANGE, or POLR_OK when all are 0
	int check_range(polr_ctx *ctx, uint64_t *n_out_of_range) const {
		uint32_t first = 0;
		const unsigned long long total = out_of_range(&first);
		if (n_out_of_range) {
			*n_out_of_range = total;
		}
		if (total) {
			POLR_FAIL(ctx, POLR_E_RANGE, "aggregate %u: %llu arguments of this call lie outside their result type (the reference: "
			          "OutOfRangeException, Overflow in addition / subtraction / multiplication); no result was written", first, total);
		}
		return POLR_OK;
	}
	uint32_t own, n;
	unsigned long long *dev = nullptr;
	unsigned long long host[MAX_OWN + POLR_MAX_AGGS] = {0};
};

// (n_out_of_range: the expression form's, may be NULL)
static int aggregate_ungrouped(polr_out *o, void *stream, SinkAggs &aggs, polr_agg_value *results, uint64_t *n_out_of_range) {
	const uint32_t n_aggs = aggs.n;
	PolrAggRequest rq = {};
	PolrAggPlan pl;
	rq.has_results = results != nullptr;
	polr_ctx *ctx = describe_sink(o, &aggs, &rq);
	POLR_TRY_SINK_PLAN(ctx, pl, polr_agg_plan_ungrouped(rq, &pl));
	build_sink_aggs(pl.agg, &aggs);
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	int rc = out_ensure_stats(o, stream);
	if (rc) {
		return rc;
	}
	const uint32_t n_blocks = std::max<uint32_t>(1, std::min<uint32_t>(o->n_chunks, (uint32_t)ctx->n_cus * 8));
	std::vector<AggPartial> host((size_t)n_blocks * n_aggs);
	SinkCounters cnt(aggs, 0);
	if (o->n_chunks) {
		DevBuf<uint8_t> mem; // the partials, and the counters behind them
		HIPCHK(ctx, mem.alloc(host.size() * sizeof(AggPartial) + cnt.bytes()));
		AggPartial *part = (AggPartial *)mem.get();
		cnt.place((unsigned long long *)(part + host.size()), &aggs);
		HIPCHK(ctx, cnt.zero(st));
		with_set(aggs, [&](const auto &set) {
			hipLaunchKernelGGL(polr_agg_kernel, dim3(n_blocks), dim3(256), 0, st, o->dev, o->n_chunks, set, part);
		});
		HIPCHK(ctx, cnt.fetch(st));
		HIPCHK(ctx, hipMemcpyAsync(host.data(), part, host.size() * sizeof(AggPartial), hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
	}
	rc = cnt.check_range(ctx, n_out_of_range);
	if (rc) {
		return rc;
	}
	for (uint32_t a = 0; a < n_aggs; a++) {
		__int128 sum = 0;
		long long mn = 0x7FFFFFFFFFFFFFFFll, mx = (long long)0x8000000000000000ull;
		unsigned long long n_rows = 0;
		for (uint32_t b = 0; b < n_blocks && o->n_chunks; b++) {
			const AggPartial &r = host[(size_t)b * n_aggs + a];
			sum += ((__int128)r.sum_hi << 64) + (__int128)r.sum_lo;
			mn = r.mn < mn ? r.mn : mn;
			mx = r.mx > mx ? r.mx : mx;
			n_rows += r.count;
		}
		results[a] = polr_agg_decode(aggs.fn[a], sum, mn, mx, n_rows);
	}
	return POLR_OK;
}

extern "C" {

int polr_out_aggregate(polr_out *o, void *stream, const polr_agg_spec *specs, uint32_t n_aggs,
                       polr_agg_value *results) {
	POLR_ENTRY();
	SinkAggs aggs(specs, n_aggs);
	return aggregate_ungrouped(o, stream, aggs, results, nullptr);
}

int polr_out_aggregate_expr(polr_out *o, void *stream, const polr_agg_expr *specs, uint32_t n_aggs, polr_agg_value *results,
                            uint64_t *n_out_of_range) {
	POLR_ENTRY();
	SinkAggs aggs(specs, n_aggs);
	return aggregate_ungrouped(o, stream, aggs, results, n_out_of_range);
}

} // extern "C"

// ---- grouped aggregate over small dense group domains (PhysicalPerfectHashAggregate's case:
// src/execution/operator/aggregate/physical_perfecthash_aggregate.cpp -- every group column has a small known
// [min, max] range, the group index is the mixed-radix number of the key offsets).  SSB Q4.x:
// GROUP BY d_year, c_nation = 7 x 25 groups.
// One accumulator cell per (group, aggregate): the sum is kept as two 64-bit limbs -- the sum of the values' low 32
// bits and the sum of their (signed) high parts -- so that plain 64-bit atomic adds stay exact for up to 2^32 rows;
// workgroups accumulate in LDS and flush their non-empty cells to the global table once.
struct GroupCell {
	unsigned long long lo32; // sum of (v & 0xFFFFFFFF)
	long long hi32;          // sum of (v >> 32), arithmetic
	long long mn, mx;
	unsigned long long count;
};

#define POLR_GROUP_LDS_CELLS 1024

__device__ __forceinline__ void cell_add(GroupCell *c, long long v) {
	atomicAdd(&c->lo32, (unsigned long long)((unsigned long long)v & 0xFFFFFFFFull));
	atomicAdd((unsigned long long *)&c->hi32, (unsigned long long)(v >> 32));
	atomicMin(&c->mn, v);
	atomicMax(&c->mx, v);
	atomicAdd(&c->count, 1ull);
}

// a cell no row has reached: the sums and the count 0, MIN / MAX at the far ends
__device__ __forceinline__ GroupCell empty_cell() {
	return GroupCell {0, 0, 0x7FFFFFFFFFFFFFFFll, (long long)0x8000000000000000ull, 0};
}

__global__ __launch_bounds__(256) void polr_group_init_kernel(GroupCell *cells, uint64_t n) {
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		cells[i] = empty_cell();
	}
}

template <class SET>
__global__ __launch_bounds__(256) void polr_group_agg_kernel(DevOut out, uint32_t n_chunks, DevGroupSet groups,
                                                             SET aggs, GroupCell *__restrict__ table,
                                                             unsigned long long *__restrict__ dropped, int use_lds) {
	typename set_traits<SET>::Oor my_oor;
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	GroupCell *local = (GroupCell *)lds_raw;
	const uint32_t n_cells = groups.n_groups * aggs.n;
	if (use_lds) {
		for (uint32_t i = threadIdx.x; i < n_cells; i += blockDim.x) {
			local[i] = empty_cell();
		}
		__syncthreads();
	}
	GroupCell *dst = use_lds ? local : table;
	unsigned long long my_dropped = 0;
	for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
		const uint32_t n = out.chunk_count[chunk];
		const uint64_t chunk_base = (uint64_t)chunk * out.chunk_capacity;
		for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
			// group index: mixed-radix number of the key offsets
			uint64_t g = 0;
			bool ok = true;
			for (uint32_t q = 0; q < groups.n; q++) {
				const DevGroupKey &gk = groups.k[q];
				const uint32_t row = out.ids[(uint64_t)gk.slot * out.slot_stride + chunk_base + i];
				if (gk.src.valid && !gk.src.valid[row]) {
					ok = false;
					break;
				}
				const long long v = load_col_cell(gk.src, row);
				const unsigned long long off = (unsigned long long)(v - gk.min_value);
				if (off >= gk.n_values) {
					ok = false;
					break;
				}
				g = g * gk.n_values + off;
			}
			if (!ok) {
				my_dropped++;
				if constexpr (set_traits<SET>::expr) { // (the reference's projection sees the row before the GROUP BY does: its range is checked)
					for (uint32_t a = 0; a < aggs.n; a++) {
						long long v;
						if (aggs.a[a].fn != POLR_AGG_COUNT_STAR) {
							arg_value(out, chunk_base + i, aggs.a[a], a, &v, &my_oor);
						}
					}
				}
				continue;
			}
			for (uint32_t a = 0; a < aggs.n; a++) {
				const auto &ag = aggs.a[a];
				GroupCell *c = &dst[g * aggs.n + a];
				if (ag.fn == POLR_AGG_COUNT_STAR) {
					atomicAdd(&c->count, 1ull);
					continue;
				}
				long long v;
				if (arg_value(out, chunk_base + i, ag, a, &v, &my_oor)) { // (NULLs take no part)
					cell_add(c, v);
				}
			}
		}
	}
	if (my_dropped) {
		atomicAdd(dropped, my_dropped);
	}
	flush_oor(aggs, my_oor);
	if (use_lds) {
		__syncthreads();
		for (uint32_t i = threadIdx.x; i < n_cells; i += blockDim.x) {
			const GroupCell c = local[i];
			if (c.count) {
				atomicAdd(&table[i].lo32, c.lo32);
				atomicAdd((unsigned long long *)&table[i].hi32, (unsigned long long)c.hi32);
				atomicMin(&table[i].mn, c.mn);
				atomicMax(&table[i].mx, c.mx);
				atomicAdd(&table[i].count, c.count);
			}
		}
	}
}

// (always inlined: the decode loops over up to 2^24 groups store straight into the caller's results)
static inline __attribute__((always_inline)) polr_agg_value cell_value(const GroupCell &c, uint32_t fn) {
	return polr_agg_decode(fn, ((__int128)c.hi32 << 32) + (__int128)c.lo32, c.mn, c.mx, c.count);
}

static int aggregate_grouped(polr_out *o, void *stream, const polr_group_key *keys, uint32_t n_keys, SinkAggs &aggs,
                             polr_agg_value *results, uint64_t n_groups, uint64_t *n_dropped, uint64_t *n_out_of_range) {
	const uint32_t n_aggs = aggs.n;
	PolrAggRequest rq = {};
	PolrAggPlan pl;
	SinkGroups cols;
	rq.has_results = results != nullptr;
	rq.n_groups = n_groups;
	polr_ctx *ctx = describe_sink(o, &aggs, &rq);
	describe_sink_groups(o, keys, n_keys, &cols, &rq);
	POLR_TRY_SINK_PLAN(ctx, pl, polr_agg_plan_grouped(rq, &pl));
	const DevGroupSet gs = dev_group_set(keys, n_keys, cols, pl.n_groups);
	build_sink_aggs(pl.agg, &aggs);
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	int rc = out_ensure_stats(o, stream);
	if (rc) {
		return rc;
	}
	const uint32_t n_cells = gs.n_groups * n_aggs;
	std::vector<GroupCell> host(n_cells);
	SinkCounters cnt(aggs, 1); // [0] dropped rows
	DevBuf<GroupCell> table_mem;
	DevBuf<uint8_t> dropped_mem;
	HIPCHK(ctx, table_mem.alloc(n_cells));
	HIPCHK(ctx, dropped_mem.alloc(cnt.bytes()));
	GroupCell *table = table_mem;
	unsigned long long *dropped = (unsigned long long *)dropped_mem.get();
	cnt.place(dropped, &aggs);
	HIPCHK(ctx, cnt.zero(st));
	hipLaunchKernelGGL(polr_group_init_kernel, dim3((n_cells + 255) / 256), dim3(256), 0, st, table, (uint64_t)n_cells);
	if (o->n_chunks) {
		const int use_lds = n_cells <= POLR_GROUP_LDS_CELLS;
		const uint32_t n_blocks = std::max<uint32_t>(1, std::min<uint32_t>(o->n_chunks, (uint32_t)ctx->n_cus * 4));
		const size_t lds = use_lds ? (size_t)n_cells * sizeof(GroupCell) : 0;
		with_set(aggs, [&](const auto &set) {
			hipLaunchKernelGGL(polr_group_agg_kernel, dim3(n_blocks), dim3(256), lds, st, o->dev, o->n_chunks, gs, set, table, dropped,
			                   use_lds);
		});
	}
	HIPCHK(ctx, hipMemcpyAsync(host.data(), table, (size_t)n_cells * sizeof(GroupCell), hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, cnt.fetch(st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	rc = cnt.check_range(ctx, n_out_of_range);
	if (rc) {
		return rc;
	}
	for (uint32_t i = 0; i < n_cells; i++) {
		results[i] = cell_value(host[i], aggs.fn[i % n_aggs]);
	}
	if (n_dropped) {
		*n_dropped = cnt.host[0];
	}
	return POLR_OK;
}

extern "C" int polr_out_aggregate_grouped(polr_out *o, void *stream, const polr_group_key *keys, uint32_t n_keys,
                                          const polr_agg_spec *specs, uint32_t n_aggs, polr_agg_value *results,
                                          uint64_t n_groups, uint64_t *n_dropped) {
	POLR_ENTRY();
	SinkAggs aggs(specs, n_aggs);
	return aggregate_grouped(o, stream, keys, n_keys, aggs, results, n_groups, n_dropped, nullptr);
}

extern "C" int polr_out_aggregate_grouped_expr(polr_out *o, void *stream, const polr_group_key *keys, uint32_t n_keys,
                                               const polr_agg_expr *specs, uint32_t n_aggs, polr_agg_value *results,
                                               uint64_t n_groups, uint64_t *n_dropped, uint64_t *n_out_of_range) {
	POLR_ENTRY();
	SinkAggs aggs(specs, n_aggs);
	return aggregate_grouped(o, stream, keys, n_keys, aggs, results, n_groups, n_dropped, n_out_of_range);
}


// ---- the GROUP BY sink fused into an emitting flat pipeline (FusedSink, polr_device.h; polr_flat_device.h) -------------
static_assert(POLR_AGG_COUNT_STAR == POLR_DEV_AGG_COUNT_STAR && POLR_AGG_COUNT == POLR_DEV_AGG_COUNT &&
                  POLR_AGG_SUM == POLR_DEV_AGG_SUM && POLR_AGG_MIN == POLR_DEV_AGG_MIN && POLR_AGG_MAX == POLR_DEV_AGG_MAX,
              "aggregate function codes");
#define POLR_FUSED_TABLES 256u // one table of group cells per workgroup (modulo): the adds of a workgroup stay among themselves

// sums the workgroup tables: out[w] += sum over the tables t = blockIdx.y, blockIdx.y + gridDim.y, ... of cells[t][w]
// (out zeroed by the caller; the table loop is split over gridDim.y for loads in flight)
__global__ __launch_bounds__(256) void polr_fused_reduce_kernel(const unsigned long long *__restrict__ cells, uint32_t n_tables,
                                                                uint32_t words, unsigned long long *__restrict__ out) {
	const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
	if (w >= words) {
		return;
	}
	unsigned long long s = 0;
	for (uint32_t t = blockIdx.y; t < n_tables; t += gridDim.y) {
		s += cells[(size_t)t * words + w];
	}
	if (s) {
		atomicAdd(&out[w], s);
	}
}

extern "C" int polr_out_fuse_grouped(polr_out *o, const polr_group_key *keys, uint32_t n_keys, const polr_agg_spec *specs,
                                     uint32_t n_aggs) {
	POLR_ENTRY();
	SinkAggs aggs(specs, n_aggs);
	PolrAggRequest rq = {};
	PolrAggPlan pl;
	SinkGroups cols;
	polr_ctx *ctx = describe_sink(o, &aggs, &rq);
	describe_sink_groups(o, keys, n_keys, &cols, &rq);
	rq.flat_emit = o && o->pipe->host_count.flat && o->pipe->flat_emit;
	POLR_TRY_SINK_PLAN(ctx, pl, polr_agg_plan_fuse_grouped(rq, &pl));
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (pl.unfuse) { // the output object collects row ids again
		if (o->fused_dev) {
			HIPCHK(ctx, hipDeviceSynchronize());
			o->fused_dev.reset();
			o->fused_cells.reset();
			o->fused_dropped.reset();
			o->dev.fused = nullptr;
		}
		return POLR_OK;
	}
	build_sink_aggs(pl.agg, &aggs);
	FusedSink fs;
	memset(&fs, 0, sizeof(fs));
	fs.groups = dev_group_set(keys, n_keys, cols, pl.n_groups);
	fs.aggs = aggs.cols;
	const uint32_t groups = fs.groups.n_groups, words = groups * polr_fused_group_words(n_aggs);
	fs.n_tables = POLR_FUSED_TABLES;
	fs.words_per_table = words;
	const size_t bytes = (size_t)(POLR_FUSED_TABLES + 1u) * words * 8u; // (+ 1: where the read-out sums the tables)
	// built in locals and moved into the output at the point of success: nothing half-made stays behind
	DevBuf<unsigned long long> cells, dropped;
	DevBuf<FusedSink> dev;
	HIPCHK(ctx, cells.alloc(bytes / 8));
	HIPCHK(ctx, dropped.alloc(1));
	HIPCHK(ctx, dev.alloc(1));
	fs.cells = cells;
	fs.dropped = dropped;
	HIPCHK(ctx, hipMemsetAsync(cells, 0, bytes, ctx->stream));
	HIPCHK(ctx, hipMemsetAsync(dropped, 0, 8, ctx->stream));
	HIPCHK(ctx, hipMemcpyAsync(dev, &fs, sizeof(fs), hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	o->fused_cells = std::move(cells);
	o->fused_dropped = std::move(dropped);
	o->fused_dev = std::move(dev);
	o->fused_tables = POLR_FUSED_TABLES;
	o->fused_groups = groups;
	o->fused_aggs = n_aggs;
	for (uint32_t a = 0; a < n_aggs; a++) {
		o->fused_fn[a] = fs.aggs.a[a].fn;
		o->fused_has_valid[a] = fs.aggs.a[a].src.valid != nullptr;
	}
	o->dev.fused = o->fused_dev;
	return POLR_OK;
}

extern "C" int polr_out_fused_result(polr_out *o, void *stream, polr_agg_value *results, uint64_t n_groups, uint64_t *n_dropped) {
	POLR_ENTRY();
	if (!o || !results) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = o->pipe->ctx;
	if (!o->fused_dev) {
		POLR_FAIL(ctx, POLR_E_INVALID, "the output object has no fused sink (polr_out_fuse_grouped)");
	}
	if (n_groups != o->fused_groups) {
		POLR_FAIL(ctx, POLR_E_INVALID, "results hold %llu groups, the sink %u", (unsigned long long)n_groups, o->fused_groups);
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	const uint32_t n_aggs = o->fused_aggs, words = o->fused_groups * polr_fused_group_words(n_aggs);
	unsigned long long *sum = o->fused_cells + (size_t)o->fused_tables * words; // (one more table behind the workgroups')
	HIPCHK(ctx, hipMemsetAsync(sum, 0, (size_t)words * 8u, st));
	hipLaunchKernelGGL(polr_fused_reduce_kernel, dim3((words + 255) / 256, 16), dim3(256), 0, st, o->fused_cells, o->fused_tables,
	                   words, sum);
	std::vector<unsigned long long> host(words);
	unsigned long long dropped = 0;
	hipError_t e = hipMemcpyAsync(host.data(), sum, (size_t)words * 8u, hipMemcpyDeviceToHost, st);
	e = e == hipSuccess ? hipMemcpyAsync(&dropped, o->fused_dropped, 8, hipMemcpyDeviceToHost, st) : e;
	e = e == hipSuccess ? hipStreamSynchronize(st) : e;
	if (e != hipSuccess) {
		POLR_FAIL(ctx, POLR_E_HIP, "fused aggregate read-out failed: %s", hipGetErrorString(e));
	}
	for (uint32_t g = 0; g < o->fused_groups; g++) {
		const unsigned long long *c = &host[(size_t)g * polr_fused_group_words(n_aggs)];
		for (uint32_t a = 0; a < n_aggs; a++) {
			const uint64_t count = o->fused_fn[a] == POLR_AGG_COUNT_STAR || !o->fused_has_valid[a] ? c[0] : c[2u + 2u * a];
			results[(size_t)g * n_aggs + a] = polr_agg_decode(o->fused_fn[a], (int64_t)c[1u + 2u * a], 0, 0, count);
		}
	}
	if (n_dropped) {
		*n_dropped = dropped;
	}
	return POLR_OK;
}

// ---- the UNGROUPED sink fused into the generic pool kernel (FusedAggSink, polr_device.h; the fold: polr_gen_device.h) ----
// What is refused, the cell layout, the reset values and the decode are polr_fuseagg_plan.h; here the output and its columns
// are described to the plan, and what it says is allocated and launched.
struct FuseAggWords { // the plan's per-word kinds and reset values, as a kernel argument
	uint8_t kind[POLR_FUSEAGG_MAX_WORDS];
	unsigned long long reset[POLR_FUSEAGG_MAX_WORDS];
};
static FuseAggWords fuseagg_words(const PolrFuseAggPlan &pl) {
	FuseAggWords w;
	memset(&w, 0, sizeof(w));
	for (uint32_t i = 0; i < pl.words_per_table; i++) {
		w.kind[i] = pl.kind[i];
		w.reset[i] = pl.reset[i];
	}
	return w;
}

// cells[t][w] = reset[w] for the n_tables tables (and the one behind them)
__global__ __launch_bounds__(256) void polr_fuseagg_fill_kernel(unsigned long long *__restrict__ cells, uint32_t n_tables,
                                                                uint32_t words, FuseAggWords ww) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < (n_tables + 1u) * words) {
		cells[i] = ww.reset[i % words];
	}
}

// cells[n_tables][w] = the tables' cells[t][w] combined by the word's rule: one wave per word, a lane takes the tables
// lane, lane + 64, ...
__global__ __launch_bounds__(64) void polr_fuseagg_combine_kernel(unsigned long long *__restrict__ cells, uint32_t n_tables,
                                                                  uint32_t words, FuseAggWords ww) {
	const uint32_t w = blockIdx.x;
	const uint32_t kind = ww.kind[w];
	unsigned long long v = ww.reset[w];
	for (uint32_t t = threadIdx.x; t < n_tables; t += 64u) {
		const unsigned long long c = cells[(size_t)t * words + w];
		v = kind == POLR_FUSEAGG_ADD ? v + c : (kind == POLR_FUSEAGG_MIN ? (c < v ? c : v) : (c > v ? c : v));
	}
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) {
		const unsigned long long c = __shfl_xor(v, d, 64);
		v = kind == POLR_FUSEAGG_ADD ? v + c : (kind == POLR_FUSEAGG_MIN ? (c < v ? c : v) : (c > v ? c : v));
	}
	if (threadIdx.x == 0) {
		cells[(size_t)n_tables * words + w] = v;
	}
}

void polr_launch_fuseagg_fill(hipStream_t st, const polr_out *o) {
	const PolrFuseAggPlan &pl = o->agg_plan;
	const uint32_t n = (pl.n_tables + 1u) * pl.words_per_table;
	hipLaunchKernelGGL(polr_fuseagg_fill_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, o->agg_cells.get(), pl.n_tables,
	                   pl.words_per_table, fuseagg_words(pl));
}

extern "C" int polr_out_fuse_aggregate(polr_out *o, const polr_agg_spec *specs, uint32_t n_aggs) {
	POLR_ENTRY();
	SinkAggs aggs(specs, n_aggs);
	PolrFuseAggRequest rq = {};
	PolrFuseAggPlan pl;
	polr_ctx *ctx = describe_sink(o, &aggs, &rq);
	if (!o) {
		return polr_fuseagg_plan(rq, &pl); // (no context to leave a message in)
	}
	POLR_TRY_PLAN(ctx, pl, polr_fuseagg_plan(rq, &pl));
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (pl.unfuse) { // the output object collects row ids again
		if (o->agg_dev) {
			HIPCHK(ctx, hipDeviceSynchronize());
			o->agg_dev.reset();
			o->agg_cells.reset();
			o->dev.agg = nullptr;
		}
		return POLR_OK;
	}
	build_sink_aggs(pl.agg, &aggs);
	FusedAggSink fs;
	memset(&fs, 0, sizeof(fs));
	fs.aggs = aggs.cols;
	fs.n_tables = pl.n_tables;
	fs.words_per_table = pl.words_per_table;
	// built in locals and moved into the output at the point of success: nothing half-made stays behind
	DevBuf<unsigned long long> cells;
	DevBuf<FusedAggSink> dev;
	HIPCHK(ctx, cells.alloc(pl.cell_words));
	HIPCHK(ctx, dev.alloc(1));
	fs.cells = cells;
	HIPCHK(ctx, hipMemcpyAsync(dev, &fs, sizeof(fs), hipMemcpyHostToDevice, ctx->stream));
	o->agg_plan = pl;
	o->agg_cells = std::move(cells);
	polr_launch_fuseagg_fill(ctx->stream, o);
	hipError_t e = hipStreamSynchronize(ctx->stream);
	if (e != hipSuccess) {
		o->agg_cells.reset();
		POLR_FAIL(ctx, POLR_E_HIP, "fused aggregate sink set-up failed: %s", hipGetErrorString(e));
	}
	o->agg_dev = std::move(dev);
	o->dev.agg = o->agg_dev;
	return POLR_OK;
}

extern "C" int polr_out_fused_aggregate_result(polr_out *o, void *stream, polr_agg_value *results, uint32_t n_aggs) {
	POLR_ENTRY();
	if (!o || !results) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = o->pipe->ctx;
	if (!o->agg_dev) {
		POLR_FAIL(ctx, POLR_E_INVALID, "the output object has no fused aggregate sink (polr_out_fuse_aggregate)");
	}
	const PolrFuseAggPlan &pl = o->agg_plan;
	if (n_aggs != pl.n_aggs) {
		POLR_FAIL(ctx, POLR_E_INVALID, "results hold %u aggregates, the sink %u", n_aggs, pl.n_aggs);
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	const uint32_t words = pl.words_per_table;
	hipLaunchKernelGGL(polr_fuseagg_combine_kernel, dim3(words), dim3(64), 0, st, o->agg_cells.get(), pl.n_tables, words,
	                   fuseagg_words(pl));
	uint64_t host[POLR_FUSEAGG_MAX_WORDS];
	hipError_t e = hipMemcpyAsync(host, o->agg_cells + (size_t)pl.n_tables * words, (size_t)words * 8u, hipMemcpyDeviceToHost, st);
	e = e == hipSuccess ? hipStreamSynchronize(st) : e;
	if (e != hipSuccess) {
		POLR_FAIL(ctx, POLR_E_HIP, "fused aggregate read-out failed: %s", hipGetErrorString(e));
	}
	char err[256];
	const int rc = polr_fuseagg_decode(pl.fn, pl.n_aggs, host, results, err, sizeof(err));
	if (rc) {
		POLR_FAIL(ctx, rc, "%s", err);
	}
	return POLR_OK;
}

// ---- the general GROUP BY sink: group columns of any integer domain or VARCHAR (PhysicalHashAggregate,
// src/execution/operator/aggregate/physical_hash_aggregate.cpp -- the plan when the group columns' statistics do not allow
// a perfect-hash aggregate; SSB: GROUP BY d_year, c_nation / c_city, s_city, d_year / p_brand) ------------------------------
// An open-addressing table of groups in global memory: state[s] = 0 empty / 1 being written / 2 ready, the group's key
// words (NULL is a group value of its own, as GROUP BY has it: a bit per column) and its cells.  A row claims an empty
// slot with a compare-and-swap and publishes its key; every other row of the group finds the key and adds to the cells.
// A lane that meets a slot "being written" does not wait inside the iteration -- the writer may be a lane of its own wave,
// which runs in lockstep -- it comes back to the slot in the next iteration of the loop all lanes share.
//
// STR (some group column is VARCHAR): such a column's key word is the 64-bit hash of the string's value, and a
// representative string_t cell sits beside it (reps[slot][column]; its pointer stays good: it points into the device heap
// the table / pipeline owns).  A probing row compares the key words -- integer values and string hashes -- and only for a
// slot that agrees in all of them the strings themselves (polr_str_equal: length, then prefix / inline characters from the
// two cells, then the heap bytes), so a slot of another group almost never costs a heap read.
//
// Few hot groups is the common shape (Q4.1: 35 groups for every surviving row).  Once every lane knows its slot, the lanes
// of a wave that resolved to the SAME slot are folded into their lowest lane -- the leader walks its peers with
// v_readlane, the work is bounded by 64 peers per wave and aggregate whatever the distribution -- and only leaders and
// lanes alone on their slot issue atomics: one per distinct slot, aggregate and wave, and only on the words cell_value
// reads for the aggregate's function.
struct HashAggTable {
	uint32_t *state;
	long long *keys;          // [capacity][n_cols]
	uint32_t *nulls;          // [capacity]: bit c = group column c is NULL
	GroupCell *cells;         // [capacity][n_aggs]
	unsigned long long *n_groups, *overflow;
	uint64_t mask;            // capacity - 1
	uint64_t max_groups;
};

#define POLR_NO_SLOT 0xFFFFFFFFu

template <bool STR, class SET>
__global__ __launch_bounds__(256) void polr_hash_agg_kernel(DevOut out, uint32_t n_chunks, DevGroupSet groups, SET aggs,
                                                            HashAggTable t, uint4 *reps, uint32_t str_mask) {
	typename set_traits<SET>::Oor my_oor;
	const uint32_t lane = threadIdx.x & 63u;
	for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
		const uint32_t n = out.chunk_count[chunk];
		const uint64_t chunk_base = (uint64_t)chunk * out.chunk_capacity;
		for (uint32_t i0 = 0; i0 < n; i0 += blockDim.x) {
			const uint32_t i = i0 + threadIdx.x;
			const bool active = i < n;
			long long key[POLR_MAX_GROUP_KEYS] = {0, 0, 0};
			uint4 cell[POLR_MAX_GROUP_KEYS]; // (STR only)
			uint32_t null_mask = 0;
			uint64_t h = 0x9E3779B97F4A7C15ull;
#pragma unroll
			for (uint32_t q = 0; q < POLR_MAX_GROUP_KEYS; q++) {
				cell[q] = make_uint4(0, 0, 0, 0);
				if (active && q < groups.n) {
					const DevGroupKey &gk = groups.k[q];
					const uint32_t row = out.ids[(uint64_t)gk.slot * out.slot_stride + chunk_base + i];
					if (gk.src.valid && !gk.src.valid[row]) {
						null_mask |= 1u << q; // (the cell of a NULL row is never read)
					} else if (STR && ((str_mask >> q) & 1u)) {
						cell[q] = ((const uint4 *)gk.src.data)[row];
						key[q] = (long long)polr_str_hash(cell[q]);
					} else {
						key[q] = load_col_cell(gk.src, row);
					}
					h = polr_murmurhash64(h ^ (uint64_t)key[q]) + q;
				}
			}
			h = polr_murmurhash64(h ^ null_mask);
			uint64_t s = h & t.mask;
			bool done = !active;
			uint64_t probes = 0;
			while (__syncthreads_or(!done)) { // (every lane of the workgroup takes part in every iteration)
				if (!done) {
					uint32_t st = __hip_atomic_load(&t.state[s], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
					if (st == 0u) {
						if (atomicCAS(&t.state[s], 0u, 1u) == 0u) {
							if (atomicAdd(t.n_groups, 1ull) >= t.max_groups) {
								atomicExch(t.overflow, 1ull); // (more groups than the caller made room for)
							}
#pragma unroll
							for (uint32_t q = 0; q < POLR_MAX_GROUP_KEYS; q++) {
								if (q < groups.n) {
									t.keys[s * groups.n + q] = key[q];
									if (STR) {
										reps[s * groups.n + q] = cell[q];
									}
								}
							}
							t.nulls[s] = null_mask;
							__hip_atomic_store(&t.state[s], 2u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
							st = 2u;
						}
					}
					if (st == 2u) {
						bool same = t.nulls[s] == null_mask;
#pragma unroll
						for (uint32_t q = 0; q < POLR_MAX_GROUP_KEYS; q++) {
							if (q < groups.n) {
								same = same && t.keys[s * groups.n + q] == key[q];
							}
						}
						if (STR && same) { // (the hashes agree: now the strings)
#pragma unroll
							for (uint32_t q = 0; q < POLR_MAX_GROUP_KEYS; q++) {
								if (q < groups.n && ((str_mask & ~null_mask) >> q) & 1u) {
									same = same && polr_str_equal(reps[s * groups.n + q], cell[q]);
								}
							}
						}
						if (same) {
							done = true;
						} else {
							s = (s + 1) & t.mask;
							if (++probes > t.mask) { // (a full table: cannot happen with capacity >= 2 x max_groups before overflow)
								atomicExch(t.overflow, 1ull);
								done = true;
								s = ~0ull;
							}
						}
					}
					// (st == 1: somebody is writing this slot's key: look again in the next iteration)
				}
			}
			// every lane of the wave is here, with its slot or none (capacity <= 2^25: a slot fits 32 bits)
			const uint32_t s32 = (active && s != ~0ull) ? (uint32_t)s : POLR_NO_SLOT;
			uint32_t lead = lane;  // the lowest lane of the wave with this lane's slot
			uint64_t shared = 0;   // the lanes whose slot another lane of the wave has too
			uint64_t todo = __ballot(s32 != POLR_NO_SLOT);
			while (todo) {
				const int l = __builtin_ctzll(todo);
				const uint32_t ls = (uint32_t)__builtin_amdgcn_readlane((int)s32, l);
				const uint64_t peers = __ballot(s32 == ls);
				if (s32 == ls) {
					lead = (uint32_t)l;
				}
				if (peers & (peers - 1)) {
					shared |= peers;
				}
				todo &= ~peers;
			}
			for (uint32_t a = 0; a < aggs.n; a++) {
				const auto &ag = aggs.a[a];
				bool have = s32 != POLR_NO_SLOT;
				long long v = 0;
				// (the expression form checks the range of a row that found no slot all the same; the plain form need not load for it)
				const bool fetch = set_traits<SET>::expr ? active : have;
				if (fetch && ag.fn != POLR_AGG_COUNT_STAR) {
					have = arg_value(out, chunk_base + i, ag, a, &v, &my_oor) && have; // (NULLs take no part)
					v = have ? v : 0;
				}
				unsigned long long cnt = have ? 1ull : 0ull, lo = (unsigned long long)v & 0xFFFFFFFFull;
				long long hi = v >> 32, mn = v, mx = v;
				uint64_t m = shared;
				while (m) {
					const int l = __builtin_ctzll(m);
					const bool mine = lead == (uint32_t)l;
					const uint64_t peers = __ballot(mine);
					const uint64_t with = __ballot(mine && have);
					unsigned long long w_lo = 0;
					long long w_hi = 0, w_mn = 0x7FFFFFFFFFFFFFFFll, w_mx = (long long)0x8000000000000000ull;
					if (ag.fn == POLR_AGG_SUM) {
						for (uint64_t b = with; b; b &= b - 1) {
							const int j = __builtin_ctzll(b);
							w_lo += (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)lo, j);
							w_hi += (long long)__builtin_amdgcn_readlane((int)hi, j); // (v >> 32 fits 32 bits)
						}
					} else if (ag.fn == POLR_AGG_MIN || ag.fn == POLR_AGG_MAX) {
						for (uint64_t b = with; b; b &= b - 1) {
							const int j = __builtin_ctzll(b);
							const long long o = (long long)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), j) << 32) |
							                                (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, j));
							w_mn = o < w_mn ? o : w_mn;
							w_mx = o > w_mx ? o : w_mx;
						}
					}
					if (mine) {
						have = lane == (uint32_t)l && with != 0; // (the leader speaks for its peers)
						cnt = (unsigned long long)__popcll(with);
						lo = w_lo;
						hi = w_hi;
						mn = w_mn;
						mx = w_mx;
					}
					m &= ~peers;
				}
				if (have) {
					GroupCell *c = &t.cells[(uint64_t)s32 * aggs.n + a];
					switch (ag.fn) { // (only the words cell_value reads for this function)
					case POLR_AGG_SUM:
						atomicAdd(&c->lo32, lo);
						atomicAdd((unsigned long long *)&c->hi32, (unsigned long long)hi);
						break;
					case POLR_AGG_MIN:
						atomicMin(&c->mn, mn);
						break;
					case POLR_AGG_MAX:
						atomicMax(&c->mx, mx);
						break;
					default:
						break;
					}
					atomicAdd(&c->count, cnt);
				}
			}
		}
	}
	flush_oor(aggs, my_oor);
}

// the groups that exist, compacted: [idx] <- slot
// (reps / reps_out: the representative string cells, or nullptr)
__global__ __launch_bounds__(256) void polr_hash_agg_compact_kernel(HashAggTable t, uint32_t n_cols, uint32_t n_aggs, long long *keys_out,
                                                                    uint32_t *nulls_out, GroupCell *cells_out, unsigned long long *cursor,
                                                                    uint64_t max_groups, const uint4 *reps, uint4 *reps_out) {
	for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= t.mask; s += (uint64_t)gridDim.x * blockDim.x) {
		if (t.state[s] != 2u) {
			continue;
		}
		const unsigned long long idx = atomicAdd(cursor, 1ull);
		if (idx >= max_groups) {
			continue;
		}
		for (uint32_t q = 0; q < n_cols; q++) {
			keys_out[idx * n_cols + q] = t.keys[s * n_cols + q];
			if (reps) {
				reps_out[idx * n_cols + q] = reps[s * n_cols + q];
			}
		}
		nulls_out[idx] = t.nulls[s];
		for (uint32_t a = 0; a < n_aggs; a++) {
			cells_out[idx * n_aggs + a] = t.cells[s * n_aggs + a];
		}
	}
}

extern "C" int polr_out_column_width(polr_out *o, int32_t src_join, uint32_t src_col, uint32_t *width) {
	POLR_ENTRY();
	if (!o || !width) {
		return POLR_E_INVALID;
	}
	OutCol c;
	int rc = polr_out_col(o->pipe, src_join, src_col, &c, "column", src_col);
	if (rc) {
		return rc;
	}
	*width = c.dev.width;
	return POLR_OK;
}

// the entry points of the general GROUP BY; strings: VARCHAR group columns are allowed, their values go to str_bytes
// (n_out_of_range: the expression form's, may be NULL)
static int aggregate_hashed(polr_out *o, void *stream, const polr_group_key *cols, uint32_t n_cols, SinkAggs &aggs,
                            uint64_t max_groups, int64_t *group_keys, uint32_t *group_nulls, polr_agg_value *results,
                            uint64_t *n_groups, bool strings, uint8_t *str_bytes, uint64_t str_cap, uint64_t *str_used,
                            uint64_t *n_out_of_range) {
	const uint32_t n_aggs = aggs.n;
	PolrAggRequest rq = {};
	PolrAggPlan pl;
	SinkGroups gcols;
	rq.has_results = results != nullptr;
	rq.has_group_outputs = group_keys && group_nulls && n_groups;
	rq.max_groups = max_groups;
	rq.strings = strings;
	rq.has_str_used = str_used != nullptr;
	rq.has_str_bytes = str_bytes != nullptr;
	rq.str_cap = str_cap;
	polr_ctx *ctx = describe_sink(o, &aggs, &rq);
	describe_sink_groups(o, cols, n_cols, &gcols, &rq);
	const int refused = polr_agg_plan_hashed(rq, &pl);
	if (strings && pl.head_passed) {
		*str_used = 0;
	}
	POLR_TRY_SINK_PLAN(ctx, pl, refused);
	const OutCol *gcol = gcols.src;
	const uint32_t str_mask = pl.str_mask;
	const DevGroupSet gs = dev_group_set(cols, n_cols, gcols, 0);
	build_sink_aggs(pl.agg, &aggs);
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	int rc = out_ensure_stats(o, stream);
	if (rc) {
		return rc;
	}
	for (uint32_t q = 0; q < n_cols; q++) { // before any kernel that follows a string pointer is enqueued
		if ((str_mask >> q) & 1u) {
			rc = check_string_col_on_device(o, st, gcol[q], "group column", q);
			if (rc) {
				return rc;
			}
		}
	}
	PolrCapacityPlan slots_plan; // (max_groups is at most 2^24: never refused)
	POLR_TRY_PLAN(ctx, slots_plan, polr_build_capacity(max_groups, slots_plan));
	const uint64_t capacity = slots_plan.capacity;
	HashAggTable t;
	memset(&t, 0, sizeof(t));
	t.mask = capacity - 1;
	t.max_groups = max_groups;
	// one allocation (polr_hashagg_layout): the table, and the compacted outputs behind it
	SinkCounters hc(aggs, SinkCounters::MAX_OWN); // [0] groups, [1] overflow, [2] compaction cursor
	PolrHashAggLayout lo;
	polr_hashagg_layout(capacity, max_groups, n_cols, n_aggs, str_mask != 0, sizeof(GroupCell), sizeof(hc.host), &lo);
	DevBuf<uint8_t> base;
	HIPCHK(ctx, base.alloc(lo.total));
	t.state = (uint32_t *)(base + lo.state);
	t.nulls = (uint32_t *)(base + lo.nulls);
	unsigned long long *cnt = (unsigned long long *)(base + lo.counters);
	hc.place(cnt, &aggs);
	t.n_groups = cnt;
	t.overflow = cnt + 1;
	t.keys = (long long *)(base + lo.keys);
	uint4 *reps = str_mask ? (uint4 *)(base + lo.reps) : nullptr;
	t.cells = (GroupCell *)(base + lo.cells);
	long long *okeys = (long long *)(base + lo.okeys);
	uint4 *oreps = str_mask ? (uint4 *)(base + lo.oreps) : nullptr;
	uint32_t *onulls = (uint32_t *)(base + lo.onulls);
	GroupCell *ocells = (GroupCell *)(base + lo.ocells);
	hipError_t e = hipMemsetAsync(base, 0, lo.zero_bytes, st); // (the counters with the table's state)
	const unsigned long long *h_cnt = hc.host;
	if (e == hipSuccess) {
		hipLaunchKernelGGL(polr_group_init_kernel, dim3(256), dim3(256), 0, st, t.cells, capacity * n_aggs);
		if (o->n_chunks) {
			const dim3 grid(std::min<uint32_t>(o->n_chunks, 2048u));
			with_set(aggs, [&](const auto &set) {
				using SET = std::decay_t<decltype(set)>;
				if (str_mask) {
					hipLaunchKernelGGL((polr_hash_agg_kernel<true, SET>), grid, dim3(256), 0, st, o->dev, o->n_chunks, gs, set, t, reps, str_mask);
				} else {
					hipLaunchKernelGGL((polr_hash_agg_kernel<false, SET>), grid, dim3(256), 0, st, o->dev, o->n_chunks, gs, set, t, reps, str_mask);
				}
			});
		}
		hipLaunchKernelGGL(polr_hash_agg_compact_kernel, dim3(256), dim3(256), 0, st, t, n_cols, n_aggs, okeys, onulls, ocells, cnt + 2,
		                   max_groups, (const uint4 *)reps, oreps);
		e = hc.fetch(st);
		e = e == hipSuccess ? hipStreamSynchronize(st) : e;
	}
	const bool too_many = h_cnt[1] || h_cnt[0] > max_groups;
	const bool out_of_range = hc.out_of_range() != 0; // (the reference's query fails: nothing is copied to the caller)
	const uint64_t g_n = too_many || out_of_range ? 0 : h_cnt[0];
	if (e != hipSuccess) {
		POLR_FAIL(ctx, POLR_E_HIP, "hash aggregate failed: %s", hipGetErrorString(e));
	}
	std::vector<GroupCell> hcells(g_n * n_aggs);
	// integer columns only: keys and NULL bits go to the caller's arrays at once; with VARCHAR columns the NULL bits are staged
	// and the keys stay on the device until the strings' records fit, so that an arena too small leaves the caller's arrays
	// as they were
	const uint64_t n_rec = str_mask ? g_n * n_cols : 0;
	std::vector<uint4> hreps(n_rec);
	std::vector<uint64_t> offs(n_rec); // the records' offsets
	std::vector<uint32_t> snulls(str_mask ? g_n : 0);
	uint32_t *hnulls = str_mask ? snulls.data() : group_nulls;
	uint64_t used = 0;
	int records = POLR_OK;
	if (g_n) {
		if (!str_mask) {
			HIPCHK(ctx, hipMemcpy(group_keys, okeys, g_n * n_cols * 8, hipMemcpyDeviceToHost));
		}
		HIPCHK(ctx, hipMemcpy(hnulls, onulls, g_n * 4, hipMemcpyDeviceToHost));
		HIPCHK(ctx, hipMemcpy(hcells.data(), ocells, g_n * n_aggs * sizeof(GroupCell), hipMemcpyDeviceToHost));
	}
	if (n_rec) {
		// the strings' records, group-major, then column: none for an integer column or a NULL value.  The offsets go up into
		// the table's own keys, which nothing reads after the compaction (capacity >= 2 x max_groups slots)
		HIPCHK(ctx, hipMemcpy(hreps.data(), oreps, n_rec * 16, hipMemcpyDeviceToHost));
		uint64_t g = 0;
		uint32_t q = 0;
		used = polr_strrec_layout(n_rec, [&](uint64_t i) { // (i = g * n_cols + q, without the division)
			const bool record = ((str_mask >> q) & 1u) && !((hnulls[g] >> q) & 1u);
			if (++q == n_cols) {
				q = 0;
				g++;
			}
			return record ? (uint64_t)hreps[i].x : POLR_STRREC_NONE;
		}, offs.data());
		records = polr_fetch_str_records(ctx, st, oreps, nullptr, n_rec, offs.data(), used, n_rec, (uint64_t *)t.keys, str_bytes, str_cap);
		if (records != POLR_OK && records != POLR_E_OVERFLOW) {
			return records;
		}
	}
	if (n_rec && records == POLR_OK) { // (with groups to report, only the arena can still be too small: it was not)
		HIPCHK(ctx, hipMemcpy(group_keys, okeys, n_rec * 8, hipMemcpyDeviceToHost));
		for (uint64_t g = 0, i = 0; g < g_n; g++) { // a VARCHAR column's key word is the offset of its record (0 for NULL)
			for (uint32_t q = 0; q < n_cols; q++, i++) {
				if ((str_mask >> q) & 1u) {
					group_keys[i] = offs[i] == POLR_STRREC_NONE ? 0 : (int64_t)offs[i];
				}
			}
		}
		memcpy(group_nulls, hnulls, g_n * 4);
	}
	rc = hc.check_range(ctx, n_out_of_range);
	if (rc) {
		return rc;
	}
	*n_groups = h_cnt[0];
	if (too_many) {
		POLR_FAIL(ctx, POLR_E_OVERFLOW, "the result has %llu groups or more, the caller made room for %llu",
		          (unsigned long long)h_cnt[0], (unsigned long long)max_groups);
	}
	if (strings) {
		*str_used = used;
	}
	if (records == POLR_E_OVERFLOW) { // (nothing was written: group_keys, group_nulls, results and str_bytes are as they were)
		POLR_FAIL(ctx, POLR_E_OVERFLOW, "the groups' strings take %llu bytes, the caller made room for %llu", (unsigned long long)used,
		          (unsigned long long)str_cap);
	}
	for (uint64_t g = 0; g < g_n; g++) {
		for (uint32_t a = 0; a < n_aggs; a++) {
			results[g * n_aggs + a] = cell_value(hcells[g * n_aggs + a], aggs.fn[a]);
		}
	}
	return POLR_OK;
}

extern "C" int polr_out_aggregate_hashed(polr_out *o, void *stream, const polr_group_key *cols, uint32_t n_cols,
                                         const polr_agg_spec *specs, uint32_t n_aggs, uint64_t max_groups, int64_t *group_keys,
                                         uint32_t *group_nulls, polr_agg_value *results, uint64_t *n_groups) {
	POLR_ENTRY();
	SinkAggs aggs(specs, n_aggs);
	return aggregate_hashed(o, stream, cols, n_cols, aggs, max_groups, group_keys, group_nulls, results, n_groups, false, nullptr, 0,
	                        nullptr, nullptr);
}

extern "C" int polr_out_aggregate_hashed_str(polr_out *o, void *stream, const polr_group_key *cols, uint32_t n_cols,
                                             const polr_agg_spec *specs, uint32_t n_aggs, uint64_t max_groups, int64_t *group_keys,
                                             uint32_t *group_nulls, polr_agg_value *results, uint64_t *n_groups, uint8_t *str_bytes,
                                             uint64_t str_cap, uint64_t *str_used) {
	POLR_ENTRY();
	SinkAggs aggs(specs, n_aggs);
	return aggregate_hashed(o, stream, cols, n_cols, aggs, max_groups, group_keys, group_nulls, results, n_groups, true, str_bytes,
	                        str_cap, str_used, nullptr);
}

extern "C" int polr_out_aggregate_hashed_expr(polr_out *o, void *stream, const polr_group_key *cols, uint32_t n_cols,
                                              const polr_agg_expr *specs, uint32_t n_aggs, uint64_t max_groups, int64_t *group_keys,
                                              uint32_t *group_nulls, polr_agg_value *results, uint64_t *n_groups,
                                              uint8_t *str_bytes, uint64_t str_cap, uint64_t *str_used, uint64_t *n_out_of_range) {
	POLR_ENTRY();
	SinkAggs aggs(specs, n_aggs);
	return aggregate_hashed(o, stream, cols, n_cols, aggs, max_groups, group_keys, group_nulls, results, n_groups, true, str_bytes,
	                        str_cap, str_used, n_out_of_range);
}
