// duckdb-polr_amd/csrc/polr_dict.hip -- dictionary encoding of a VARCHAR payload column of a build side
// or of a probe column of a pipeline (polr_ht_encode_dictionary[_ex] / polr_ht_fetch_dictionary[_codes],
// polr_pipeline_encode_dictionary / polr_pipeline_fetch_dictionary[_codes] of include/polr_hip.h).
//
// A group column that is a payload column of a build side has at most as many distinct values as the build side has rows,
// and the build side is uploaded once: the strings are hashed and compared ONCE PER BUILD ROW here, at build time, and the
// column becomes dense 4-byte codes -- an ordinary integer payload column for the perfect-hash sink and the fused sink
// (polr_out_aggregate_grouped, polr_out_fuse_grouped), whose probe side then reads one 4-byte cell per surviving tuple.
//
// Codes are deterministic: the code of a value is the number of distinct non-NULL values whose first occurrence (lowest
// build row) comes before its own, i.e. 0 .. n_codes - 1 in order of first appearance; NULL rows get n_codes.  Three
// steps over the build rows, all on the device, nothing read back before the final count:
//   insert  every non-NULL row finds or claims the slot of its string in an open-addressing table (capacity a power of two
//           >= 2 x rows) and lowers the slot's first_row to its own row number;
//   rank    row r is a first occurrence iff first_row[slot_of_row[r]] == r; an exclusive prefix sum of that flag over the
//           rows is the first occurrence's code, the total is n_codes;
//   assign  code[r] = the code of r's slot, NULL rows n_codes.
//
// POLR_DICT_SORTED (polr_ht_encode_dictionary_ex): the codes rise with the strings, in the order of polr_strcmp.h.  Once
// n_codes is known the representative cells are sorted on the device and the first-appearance codes renumbered before the
// assign step:
//   keys      per code a 16-byte record {first 8 bytes of the string as a big-endian number, zero-padded; code; length} and
//             a copy of its cell.  Two records whose keys differ are ordered by the keys (masked big-endian words,
//             polr_strcmp.h); equal keys with a string of at most 8 bytes among them are ordered by length (the shorter is
//             a prefix of the other); only then are the cells compared (polr_str_cell_cmp3).
//   tile sort a workgroup sorts POLR_DICT_SORT_TILE records in LDS with a bitonic network (a last, short tile: the network
//             of the next power of two).  n_codes <= one tile: this is the whole sort.
//   merge     ping-pong buffers, every pass doubles the run length.  A workgroup produces one tile of output: it finds its
//             split of the two input runs by a binary search on the merge diagonal, loads that many records into LDS, and
//             every thread merges POLR_DICT_SORT_TILE / 256 of them from its own diagonal.  An unpaired last run is copied.
//   renumber  rank[old code] = sorted position, the representative cells in sorted order; assign writes rank[...].
// Workgroups meet at kernel boundaries only; every loop is bounded by the tile size, log2(n_codes) or a string's length.
// Distinct values never compare equal, so the result is unique whatever the network does with the padding records.
//
// A VARCHAR PROBE column is encoded by the same steps (polr_pipeline_encode_dictionary), and becomes an ordinary 4-byte
// probe column of its pipeline.  Probe tables are the large ones and their sources are usually filtered, so the call has a
// mode over the selection in force (POLR_DICT_SELECTED): the insert step and the heap guard read r = sel[i] for the
// positions of the selection and no other row, the string table is sized by the selected count, and slot_of_row starts as
// "no slot" everywhere, so that rank and assign -- which run over the table's rows -- give the rows outside the selection
// the NULL code.  A selection may be in any order and name a row twice: the insert lowers first_row by a wave reduction
// over the lanes on a slot, not by the lowest lane.
//
// The host side follows polr_dict_plan.h and polr_pdict_plan.h: the refusals of a request, what the device's answer means,
// the layout of the scratch and of the sort's, the tile sizes.  The dictionary's strings leave the device as the records
// of polr_strrec_plan.h, by polr_fetch_str_records (polr_strheap.hip).
#include <algorithm>
#include <cstring>

#include "polr_dict_plan.h"
#include "polr_internal.h"
#include "polr_pdict_plan.h"
#include "polr_strcmp.h"
#include "polr_strrec_plan.h"

#define POLR_DICT_NO_SLOT 0xFFFFFFFFu

struct DictTable {
	uint32_t *state;     // [capacity] 0 empty / 1 being written / 2 ready
	uint64_t *hash;      // [capacity] polr_str_hash of the slot's string
	uint4 *rep;          // [capacity] the claimer's cell
	uint32_t *first_row; // [capacity] lowest build row that holds the slot's string (0xFFFFFFFF: none yet)
	uint32_t *code;      // [capacity] the slot's code (rank step)
	uint64_t mask;       // capacity - 1
};

// scalars: [0] n_codes, [1] some row is NULL, [2] the table was full (cannot happen: capacity >= 2 x rows)
enum { DICT_N_CODES = 0, DICT_HAS_NULL = 1, DICT_FULL = 2, DICT_SCALARS = 4 };

__global__ __launch_bounds__(256) void polr_dict_init_kernel(DictTable t) {
	for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= t.mask; s += (uint64_t)gridDim.x * blockDim.x) {
		t.state[s] = 0u;
		t.first_row[s] = 0xFFFFFFFFu;
	}
}

// the guard of a column whose cells were never rebased onto a device heap: its non-NULL cells longer than 12 bytes (their
// pointers are the host's).  Reads the length word of a cell and nothing else.  SEL: the rows are those of sel[0 .. n), a row
// counted once per position that lists it.
template <bool SEL>
__global__ __launch_bounds__(256) void polr_dict_count_long_kernel(const uint4 *__restrict__ cells, const uint8_t *__restrict__ valid,
                                                                   const uint32_t *__restrict__ sel, uint64_t n_rows, uint64_t n,
                                                                   unsigned long long *__restrict__ n_long) {
	unsigned long long mine = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t r = SEL ? sel[i] : i;
		if (r >= n_rows || (valid && !valid[r])) { // (a position that names no row of the table selects nothing)
			continue;
		}
		mine += *(const uint32_t *)(cells + r) > 12u ? 1u : 0u;
	}
	mine = wave_sum64(mine);
	if ((threadIdx.x & 63u) == 0 && mine) {
		atomicAdd(n_long, mine);
	}
}

// true in the lowest lane of every set of lanes that `want` it and hold the same value; to be called by all lanes of the
// wave.  One step per distinct value among those lanes: few distinct values is the common shape.
__device__ __forceinline__ bool dict_first_of_equals(uint32_t v, bool want, uint32_t lane) {
	uint64_t todo = __ballot(want);
	bool first = false;
	while (todo) {
		const int l = __builtin_ctzll(todo);
		const uint32_t lv = (uint32_t)__builtin_amdgcn_readlane((int)v, l);
		first = first || lane == (uint32_t)l;
		todo &= ~__ballot(want && v == lv);
	}
	return first;
}

__device__ __forceinline__ uint32_t wave_min32(uint32_t v) { // the same minimum in every lane
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) {
		v = min(v, (uint32_t)__shfl_xor((int)v, d, 64));
	}
	return v;
}

// of every set of lanes that `want` it and hold the same value v: the minimum of their x, returned in the lowest lane of the
// set; 0xFFFFFFFF in every other lane (x is below that: a row number).  To be called by all lanes of the wave.  One
// reduction per distinct value among those lanes.
__device__ __forceinline__ uint32_t dict_min_of_equals(uint32_t v, uint32_t x, bool want) {
	const uint32_t lane = threadIdx.x & 63u;
	uint64_t todo = __ballot(want);
	uint32_t out = 0xFFFFFFFFu;
	while (todo) {
		const int l = __builtin_ctzll(todo);
		const uint32_t lv = (uint32_t)__builtin_amdgcn_readlane((int)v, l);
		const bool mine = want && v == lv;
		const uint32_t low = wave_min32(mine ? x : 0xFFFFFFFFu);
		out = lane == (uint32_t)l ? low : out;
		todo &= ~__ballot(mine);
	}
	return out;
}

// insert: the claim protocol of the general GROUP BY sink (polr_hash_agg_kernel, polr_agg.hip): a row claims an empty slot
// with a compare-and-swap, writes hash and cell, and publishes them with a release store of state 2; every other row reads
// the state with an acquire load.  A lane that meets a slot "being written" does not wait inside the iteration -- the writer
// may be a lane of its own wave, which runs in lockstep -- it looks again in the next iteration of the loop all lanes share.
// Few distinct values is the common shape (5 nations over millions of customers): hash + one slot read + one comparison.
//
// SEL: position i of sel[0 .. n) inserts table row sel[i] (the selection in force: a scan's result ascends, a host's list
// is in any order and may name a row twice); rows the selection does not name are never read, and their slot_of_row is what
// the host put there.
template <bool SEL>
__global__ __launch_bounds__(256) void polr_dict_insert_kernel(const uint4 *__restrict__ cells, const uint8_t *__restrict__ valid,
                                                               const uint32_t *__restrict__ sel, uint64_t n_rows, uint64_t n, DictTable t,
                                                               uint32_t *__restrict__ slot_of_row, uint32_t *__restrict__ scalars) {
	const uint32_t lane = threadIdx.x & 63u;
	// (every thread of a workgroup makes the same number of trips: the probe loop below is a workgroup-wide one)
	for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t i = base + threadIdx.x;
		const uint64_t r = SEL ? (i < n ? (uint64_t)sel[i] : n_rows) : i;
		const bool in_range = SEL ? r < n_rows : r < n; // (a position that names no row of the table selects nothing)
		const bool is_null = in_range && valid && !valid[r];
		const bool active = in_range && !is_null;
		uint4 cell = make_uint4(0, 0, 0, 0);
		uint64_t h = 0;
		if (active) { // (the cell of a NULL row is never read)
			cell = cells[r];
			h = polr_str_hash(cell);
		}
		if (__ballot(is_null) && lane == 0) {
			atomicOr(&scalars[DICT_HAS_NULL], 1u);
		}
		uint64_t s = h & t.mask;
		bool done = !active;
		uint64_t probes = 0;
		while (__syncthreads_or(!done)) {
			const uint32_t st = done ? 3u : __hip_atomic_load(&t.state[s], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
			// (of the lanes of a wave that found the same slot empty, one tries to claim it: a fresh table is not hit by
			// one compare-and-swap per row)
			if (dict_first_of_equals((uint32_t)s, st == 0u, lane)) {
				if (atomicCAS(&t.state[s], 0u, 1u) == 0u) {
					t.hash[s] = h;
					t.rep[s] = cell;
					__hip_atomic_store(&t.state[s], 2u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
					done = true;
				}
			} else if (st == 2u) {
				if (t.hash[s] == h && polr_str_equal(t.rep[s], cell)) {
					done = true;
				} else {
					s = (s + 1) & t.mask;
					if (++probes > t.mask) {
						atomicOr(&scalars[DICT_FULL], 1u);
						done = true;
						s = ~0ull;
					}
				}
			}
			// (an empty slot left to another lane, st == 1, or the compare-and-swap lost: somebody is writing this slot:
			// look again in the next iteration)
		}
		const uint32_t s32 = (active && s != ~0ull) ? (uint32_t)s : POLR_DICT_NO_SLOT;
		if (in_range) {
			slot_of_row[r] = s32;
		}
		// first_row[slot] = min over the slot's rows.  A row not below the value already there has nothing to add; of the
		// others, rows rise with the lane, so the lowest lane of the wave on a slot speaks for all of them: one atomic per
		// wave and distinct slot at most, whatever the distribution (every row on one slot: one per wave).
		const bool below = s32 != POLR_DICT_NO_SLOT &&
		                   (uint32_t)r < __hip_atomic_load(&t.first_row[s32], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (!SEL) {
			if (dict_first_of_equals(s32, below, lane)) {
				atomicMin(&t.first_row[s32], (uint32_t)r);
			}
		} else {
			// through a selection the rows do NOT rise with the lane: the lanes on a slot are reduced to their lowest row, which
			// the first of them sends -- still one atomic per wave and distinct slot at most
			const uint32_t low = dict_min_of_equals(s32, (uint32_t)r, below);
			if (low != 0xFFFFFFFFu) {
				atomicMin(&t.first_row[s32], low);
			}
		}
	}
}

__device__ __forceinline__ bool dict_is_first(const DictTable &t, const uint32_t *__restrict__ slot_of_row, uint64_t r, uint64_t n) {
	if (r >= n) {
		return false;
	}
	const uint32_t s = slot_of_row[r];
	return s != POLR_DICT_NO_SLOT && t.first_row[s] == (uint32_t)r;
}

// rank, pass 1: first occurrences per 1024 rows
__global__ __launch_bounds__(256) void polr_dict_rank_reduce_kernel(DictTable t, const uint32_t *__restrict__ slot_of_row, uint64_t n,
                                                                    uint32_t *__restrict__ block_sums) {
	__shared__ uint32_t wave_sum[POLR_DICT_BLOCK / 64];
	const uint64_t base = (uint64_t)blockIdx.x * POLR_DICT_BLOCK * POLR_DICT_ITEMS;
	uint32_t mine = 0;
	for (uint32_t i = 0; i < POLR_DICT_ITEMS; i++) {
		mine += (uint32_t)__popcll(__ballot(dict_is_first(t, slot_of_row, base + i * POLR_DICT_BLOCK + threadIdx.x, n)));
	}
	if ((threadIdx.x & 63u) == 0) {
		wave_sum[threadIdx.x >> 6] = mine; // (the ballots' counts: the same in every lane)
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t sum = 0;
		for (uint32_t w = 0; w < POLR_DICT_BLOCK / 64; w++) {
			sum += wave_sum[w];
		}
		block_sums[blockIdx.x] = sum;
	}
}

// rank, pass 3 (pass 2: the block-sum scan of polr_build.hip): every first occurrence gets its code = the first occurrences
// before it; the code goes to its slot, its row to row_of_code[code] (where the representative cells are taken from)
__global__ __launch_bounds__(256) void polr_dict_rank_apply_kernel(DictTable t, const uint32_t *__restrict__ slot_of_row, uint64_t n,
                                                                   const uint32_t *__restrict__ block_sums,
                                                                   uint32_t *__restrict__ row_of_code) {
	__shared__ uint32_t wave_sum[POLR_DICT_BLOCK / 64];
	const uint32_t wave = threadIdx.x >> 6;
	const uint64_t base = (uint64_t)blockIdx.x * POLR_DICT_BLOCK * POLR_DICT_ITEMS;
	uint32_t run = block_sums[blockIdx.x];
	for (uint32_t i = 0; i < POLR_DICT_ITEMS; i++) {
		const uint64_t r = base + i * POLR_DICT_BLOCK + threadIdx.x;
		const bool first = dict_is_first(t, slot_of_row, r, n);
		const uint64_t firsts = __ballot(first);
		if ((threadIdx.x & 63u) == 0) {
			wave_sum[wave] = (uint32_t)__popcll(firsts);
		}
		__syncthreads();
		uint32_t before = 0, all = 0;
		for (uint32_t w = 0; w < POLR_DICT_BLOCK / 64; w++) {
			before += w < wave ? wave_sum[w] : 0u;
			all += wave_sum[w];
		}
		if (first) {
			const uint32_t code = run + before + lane_rank(firsts);
			t.code[slot_of_row[r]] = code;
			row_of_code[code] = (uint32_t)r;
		}
		run += all;
		__syncthreads(); // (wave_sum is written again in the next round)
	}
}

// assign: the code column.  rank (sorted codes; NULL: none): the sorted position of every first-appearance code
__global__ __launch_bounds__(256) void polr_dict_assign_kernel(DictTable t, const uint32_t *__restrict__ slot_of_row, uint64_t n,
                                                               const uint32_t *__restrict__ scalars, const uint32_t *__restrict__ rank,
                                                               uint32_t *__restrict__ codes) {
	const uint32_t n_codes = scalars[DICT_N_CODES];
	for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t s = slot_of_row[r];
		codes[r] = s == POLR_DICT_NO_SLOT ? n_codes : (rank ? rank[t.code[s]] : t.code[s]);
	}
}

// the representative cell of every code: the cell of its first occurrence
__global__ __launch_bounds__(256) void polr_dict_reps_kernel(const uint4 *__restrict__ cells, const uint32_t *__restrict__ row_of_code,
                                                             uint32_t n_codes, uint4 *__restrict__ reps) {
	const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c < n_codes) {
		reps[c] = cells[row_of_code[c]];
	}
}

// POLR_DICT_SELECTED | POLR_DICT_NULL_INVALID: the code column's validity array is `valid AND selected`.  The host has
// written zeros; every position of the selection writes its row's validity (1 where the source has no array).
__global__ __launch_bounds__(256) void polr_dict_sel_valid_kernel(const uint8_t *__restrict__ valid, const uint32_t *__restrict__ sel,
                                                                  uint64_t n_rows, uint64_t n, uint8_t *__restrict__ out) {
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t r = sel[i];
		if (r < n_rows) {
			out[r] = valid ? valid[r] : (uint8_t)1;
		}
	}
}

// ---- POLR_DICT_SORTED: the sort of the representative cells -----------------------------------------------------------------
#define POLR_DICT_SORT_ITEMS (POLR_DICT_SORT_TILE / POLR_DICT_BLOCK) // records a thread merges
#define POLR_DICT_PAD 0xFFFFFFFFu // the code of a padding record: behind every string
static_assert(POLR_DICT_SORT_TILE * 16u <= 32u * 1024u, "a tile is at most 32 KB of LDS");
static_assert((POLR_DICT_SORT_TILE & (POLR_DICT_SORT_TILE - 1u)) == 0 && POLR_DICT_SORT_TILE % POLR_DICT_BLOCK == 0,
              "a tile is a power of two and a whole number of records per thread");

struct alignas(16) DictRec {
	uint64_t key;  // bytes 0-7 of the string as a big-endian number, zero beyond its length
	uint32_t code; // first-appearance code
	uint32_t len;
};
static_assert(sizeof(DictRec) == POLR_DICT_REC_BYTES, "polr_dict_sort_layout lays out records of this size");

// a < b in the order of polr_strcmp.h.  rep_old: the cell of every first-appearance code
__device__ __forceinline__ bool dict_rec_less(const DictRec &a, const DictRec &b, const uint4 *__restrict__ rep_old) {
	if (a.code == POLR_DICT_PAD || b.code == POLR_DICT_PAD) {
		return a.code != POLR_DICT_PAD;
	}
	if (a.key != b.key) {
		return a.key < b.key;
	}
	if (a.len <= 8u || b.len <= 8u) {
		return a.len < b.len; // (equal keys: the string that ends inside them is a prefix of the other)
	}
	const uint4 x = rep_old[a.code], y = rep_old[b.code];
	return polr_str_cell_cmp3(x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w) < 0;
}

// keys: the record and the cell of every first-appearance code.  The one place that reads bytes 4-7 of a long string.
__global__ __launch_bounds__(256) void polr_dict_sort_keys_kernel(const uint4 *__restrict__ cells, const uint32_t *__restrict__ row_of_code,
                                                                  uint32_t n_codes, uint4 *__restrict__ rep_old, DictRec *__restrict__ recs) {
	const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= n_codes) {
		return;
	}
	const uint4 cell = cells[row_of_code[c]];
	rep_old[c] = cell;
	const uint32_t hi = polr_str_bswap(cell.y & polr_str_word_mask(cell.x, 0));
	uint32_t lo;
	if (cell.x <= 12u) {
		lo = polr_str_bswap(cell.z & polr_str_word_mask(cell.x, 1));
	} else {
		const POLR_STRCMP_MEM uint8_t *p = (const POLR_STRCMP_MEM uint8_t *)(((uint64_t)cell.w << 32) | cell.z);
		lo = ((uint32_t)p[4] << 24) | ((uint32_t)p[5] << 16) | ((uint32_t)p[6] << 8) | (uint32_t)p[7];
	}
	DictRec r;
	r.key = ((uint64_t)hi << 32) | lo;
	r.code = c;
	r.len = cell.x;
	recs[c] = r;
}

// tile sort: records [blockIdx.x * TILE, + TILE) of recs, in place.  A short last tile is padded to the next power of two
// with records that sort behind every string, and only its own records are written back.
__global__ __launch_bounds__(256) void polr_dict_sort_tile_kernel(DictRec *recs, uint32_t n_codes, const uint4 *__restrict__ rep_old) {
	__shared__ DictRec tile[POLR_DICT_SORT_TILE];
	const uint32_t base = blockIdx.x * POLR_DICT_SORT_TILE;
	const uint32_t count = min(POLR_DICT_SORT_TILE, n_codes - base);
	uint32_t m = 2;
	while (m < count) {
		m <<= 1;
	}
	for (uint32_t i = threadIdx.x; i < m; i += POLR_DICT_BLOCK) {
		DictRec r;
		if (i < count) {
			r = recs[base + i];
		} else {
			r.key = ~0ull;
			r.code = POLR_DICT_PAD;
			r.len = 0;
		}
		tile[i] = r;
	}
	__syncthreads();
	for (uint32_t k = 2; k <= m; k <<= 1) {
		for (uint32_t j = k >> 1; j; j >>= 1) {
			for (uint32_t t = threadIdx.x; t < m / 2; t += POLR_DICT_BLOCK) {
				const uint32_t lo = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), hi = lo | j;
				const bool up = (lo & k) == 0;
				const DictRec a = tile[lo], b = tile[hi];
				if (dict_rec_less(b, a, rep_old) == up) { // (up: b < a is out of order; down: a <= b is)
					tile[lo] = b;
					tile[hi] = a;
				}
			}
			__syncthreads();
		}
	}
	for (uint32_t i = threadIdx.x; i < count; i += POLR_DICT_BLOCK) {
		recs[base + i] = tile[i];
	}
}

// how many of the first d records of the merge of A and B come from A (on a tie A goes first; strings never tie)
template <class Recs>
__device__ __forceinline__ uint32_t dict_merge_split(Recs A, uint32_t len_a, Recs B, uint32_t len_b, uint32_t d,
                                                     const uint4 *__restrict__ rep_old) {
	uint32_t lo = d > len_b ? d - len_b : 0u, hi = min(d, len_a);
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (dict_rec_less(B[d - 1u - mid], A[mid], rep_old)) {
			hi = mid;
		} else {
			lo = mid + 1u;
		}
	}
	return lo;
}

// merge pass: `in` is sorted in runs of `run` records (a multiple of the tile; the last run may be short), `out` gets runs
// of 2 x run.  Workgroup b writes out[b * TILE, + TILE): one pair of runs holds it, since 2 x run is a multiple of the tile.
__global__ __launch_bounds__(256) void polr_dict_sort_merge_kernel(const DictRec *__restrict__ in, DictRec *__restrict__ out, uint32_t n_codes,
                                                                   uint32_t run, const uint4 *__restrict__ rep_old) {
	__shared__ DictRec tile[POLR_DICT_SORT_TILE];
	__shared__ uint32_t split[2];
	const uint32_t o0 = blockIdx.x * POLR_DICT_SORT_TILE;
	const uint32_t a_start = o0 - o0 % (2u * run);
	const uint32_t len_a = min(run, n_codes - a_start);
	const uint32_t b_start = a_start + len_a;
	const uint32_t len_b = min(run, n_codes - b_start);
	const uint32_t d0 = o0 - a_start, d1 = min(d0 + POLR_DICT_SORT_TILE, len_a + len_b);
	const DictRec *A = in + a_start, *B = in + b_start;
	if (len_b == 0) { // an unpaired last run
		for (uint32_t i = d0 + threadIdx.x; i < d1; i += POLR_DICT_BLOCK) {
			out[a_start + i] = A[i];
		}
		return;
	}
	if (threadIdx.x == 0 || threadIdx.x == 64) { // (two waves, one diagonal each)
		split[threadIdx.x >> 6] = dict_merge_split(A, len_a, B, len_b, threadIdx.x ? d1 : d0, rep_old);
	}
	__syncthreads();
	const uint32_t a0 = split[0], b0 = d0 - a0, na = split[1] - a0, count = d1 - d0, nb = count - na;
	for (uint32_t i = threadIdx.x; i < count; i += POLR_DICT_BLOCK) {
		tile[i] = i < na ? A[a0 + i] : B[b0 + (i - na)];
	}
	__syncthreads();
	const DictRec *ta = tile, *tb = tile + na;
	const uint32_t d = min(threadIdx.x * POLR_DICT_SORT_ITEMS, count), dn = min(d + POLR_DICT_SORT_ITEMS, count);
	uint32_t ai = dict_merge_split(ta, na, tb, nb, d, rep_old), bi = d - ai;
	for (uint32_t o = d; o < dn; o++) {
		const bool from_a = bi >= nb || (ai < na && !dict_rec_less(tb[bi], ta[ai], rep_old));
		out[o0 + o] = from_a ? ta[ai++] : tb[bi++];
	}
}

// renumber: the representative cells in sorted order, and the sorted position of every first-appearance code
__global__ __launch_bounds__(256) void polr_dict_renumber_kernel(const DictRec *__restrict__ sorted, const uint4 *__restrict__ rep_old,
                                                                 uint32_t n_codes, uint4 *__restrict__ reps, uint32_t *__restrict__ rank) {
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= n_codes) {
		return;
	}
	const uint32_t c = sorted[p].code;
	if (c < n_codes) { // (a permutation of the codes: always)
		reps[p] = rep_old[c];
		rank[c] = p;
	}
}

// the length of the string of every listed code (each below n_codes: the host checked)
__global__ __launch_bounds__(256) void polr_dict_lens_kernel(const uint4 *__restrict__ reps, const uint32_t *__restrict__ codes, uint32_t n,
                                                             uint32_t *__restrict__ lens) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) {
		lens[i] = reps[codes[i]].x;
	}
}

static uint32_t dict_grid(uint64_t n, int n_cus) {
	return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)n_cus * 8));
}

// What the two encode calls ask of the encoder they share (dict_encode): the plan's answer and the column.  sel: the
// positions inserted (POLR_DICT_SELECTED with a selection in force), NULL: every row.
struct DictJob {
	const PolrDictPlan *pl;  // sorted, null_invalid, capacity
	const OwnedCol *src;     // the VARCHAR column, of n_rows rows
	uint64_t n_rows;
	const uint32_t *sel;     // device, n_insert positions
	uint64_t n_insert;       // sel == NULL: n_rows
	uint32_t col;            // the column's number, for the refusals
	bool probe;              // a probe column: the refusals in the pipeline's words (polr_pdict_plan.h)
};

static int dict_outcome(const DictJob &job, const char *hip_error, unsigned long long n_long, bool full, PolrPDictPlan *pl) {
	return job.probe ? polr_pdict_plan_outcome(hip_error, n_long, full, job.col, pl) : polr_dict_plan_outcome(hip_error, n_long, full, job.col, pl);
}

// The encoder: the code column (and its validity array, where it gets one) into `codes`, the counts and the representative
// cells into `d`.  Allocates, launches and waits; touches no handle -- the caller commits what it returns, or nothing.
static int dict_encode(polr_ctx *ctx, hipStream_t st, const DictJob &job, OwnedCol &codes, DictCol &d) {
	PolrPDictPlan pl = PolrPDictPlan(); // (the text of a refusal of the device's answer)
	pl.sorted = job.pl->sorted;
	pl.null_invalid = job.pl->null_invalid;
	pl.capacity = job.pl->capacity;
	const OwnedCol &src = *job.src;
	const uint64_t n = job.n_rows, n_insert = job.n_insert;
	const uint4 *cells = (const uint4 *)src.data;
	const uint8_t *valid = src.valid;
	const uint32_t *sel = job.sel;
	// allocate: the code column and one scratch allocation.  Everything lives in the caller's scope or in this one: a
	// failure frees it
	codes.width = 4;
	codes.flags = 0;
	HIPCHK(ctx, codes.alloc_data(polr_build_buffer_bytes(n * 4))); // (what polr_ht_export reports for the column)
	if (pl.null_invalid && sel) {
		// through a selection: `valid AND selected`, also for a source without a validity array
		HIPCHK(ctx, codes.alloc_valid(n));
		if (n) {
			HIPCHK(ctx, hipMemsetAsync(codes.valid, 0, n, st));
		}
		if (n_insert) {
			hipLaunchKernelGGL(polr_dict_sel_valid_kernel, dim3(dict_grid(n_insert, ctx->n_cus)), dim3(256), 0, st, valid, sel, n, n_insert,
			                   codes.valid);
		}
	} else if (pl.null_invalid && valid) { // the code column's own copy of the validity array
		HIPCHK(ctx, codes.alloc_valid(n));
		if (n) {
			HIPCHK(ctx, hipMemcpyAsync(codes.valid, valid, n, hipMemcpyDeviceToDevice, st));
		}
	}
	PolrDictLayout lo;
	if (sel) {
		polr_pdict_layout(pl.capacity, n, n_insert, &lo);
	} else {
		polr_dict_layout(pl.capacity, n, &lo);
	}
	DevBuf<uint8_t> base;
	HIPCHK(ctx, base.alloc(lo.total));
	DictTable t;
	t.rep = (uint4 *)(base + lo.rep);
	t.hash = (uint64_t *)(base + lo.hash);
	t.state = (uint32_t *)(base + lo.state);
	t.first_row = (uint32_t *)(base + lo.first_row);
	t.code = (uint32_t *)(base + lo.code);
	t.mask = pl.capacity - 1;
	uint32_t *slot_of_row = (uint32_t *)(base + lo.slot_of_row);
	uint32_t *row_of_code = (uint32_t *)(base + lo.row_of_code);
	uint32_t *block_sums = (uint32_t *)(base + lo.block_sums);
	uint32_t *scalars = (uint32_t *)(base + lo.scalars);
	// heap guard: the library uploaded the column and its heap never came: inline strings only, checked before a pointer is
	// followed
	if (n_insert && src.owned() && !src.strings_rebased) {
		unsigned long long *n_long = (unsigned long long *)(base + lo.n_long), h_long = 0;
		HIPCHK(ctx, hipMemsetAsync(n_long, 0, 8, st));
		if (sel) {
			hipLaunchKernelGGL(polr_dict_count_long_kernel<true>, dim3(dict_grid(n_insert, ctx->n_cus)), dim3(256), 0, st, cells, valid, sel, n,
			                   n_insert, n_long);
		} else {
			hipLaunchKernelGGL(polr_dict_count_long_kernel<false>, dim3(dict_grid(n, ctx->n_cus)), dim3(256), 0, st, cells, valid,
			                   (const uint32_t *)nullptr, n, n, n_long);
		}
		HIPCHK(ctx, hipMemcpyAsync(&h_long, n_long, 8, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		POLR_TRY_PLAN(ctx, pl, dict_outcome(job, nullptr, h_long, false, &pl));
	}
	// build: insert and rank; first-appearance codes are assigned at once.  Through a selection the rows it does not name
	// start, and stay, without a slot: the rank and assign steps run over the table's rows as they are
	HIPCHK(ctx, hipMemsetAsync(scalars, 0, DICT_SCALARS * 4, st));
	if (n) {
		hipLaunchKernelGGL(polr_dict_init_kernel, dim3(dict_grid(pl.capacity, ctx->n_cus)), dim3(256), 0, st, t);
		if (sel) {
			HIPCHK(ctx, hipMemsetAsync(slot_of_row, 0xFF, n * 4, st)); // (POLR_DICT_NO_SLOT)
			hipLaunchKernelGGL(polr_dict_insert_kernel<true>, dim3(dict_grid(n_insert, ctx->n_cus)), dim3(256), 0, st, cells, valid, sel, n,
			                   n_insert, t, slot_of_row, scalars);
		} else {
			hipLaunchKernelGGL(polr_dict_insert_kernel<false>, dim3(dict_grid(n, ctx->n_cus)), dim3(256), 0, st, cells, valid,
			                   (const uint32_t *)nullptr, n, n, t, slot_of_row, scalars);
		}
		hipLaunchKernelGGL(polr_dict_rank_reduce_kernel, dim3(lo.n_blocks), dim3(POLR_DICT_BLOCK), 0, st, t, (const uint32_t *)slot_of_row,
		                   n, block_sums);
		polr_launch_scan_blocksums(st, block_sums, lo.n_blocks, &scalars[DICT_N_CODES]);
		hipLaunchKernelGGL(polr_dict_rank_apply_kernel, dim3(lo.n_blocks), dim3(POLR_DICT_BLOCK), 0, st, t, (const uint32_t *)slot_of_row,
		                   n, (const uint32_t *)block_sums, row_of_code);
		if (!pl.sorted) {
			hipLaunchKernelGGL(polr_dict_assign_kernel, dim3(dict_grid(n, ctx->n_cus)), dim3(256), 0, st, t, (const uint32_t *)slot_of_row, n,
			                   (const uint32_t *)scalars, (const uint32_t *)nullptr, (uint32_t *)codes.data);
		}
	}
	// count: the one read-back of the scalars
	uint32_t h_scalars[DICT_SCALARS] = {0, 0, 0, 0};
	hipError_t e = hipMemcpyAsync(h_scalars, scalars, sizeof(h_scalars), hipMemcpyDeviceToHost, st);
	e = e == hipSuccess ? hipStreamSynchronize(st) : e;
	POLR_TRY_PLAN(ctx, pl, dict_outcome(job, e != hipSuccess ? hipGetErrorString(e) : nullptr, 0, h_scalars[DICT_FULL] != 0, &pl));
	d.n_codes = h_scalars[DICT_N_CODES];
	d.has_null = h_scalars[DICT_HAS_NULL];
	// sort (sorted codes, two values or more) or representatives
	DevBuf<uint8_t> sort_mem;
	const uint32_t *rank = nullptr;
	if (d.n_codes) {
		HIPCHK(ctx, d.cells.alloc(d.n_codes));
	}
	if (pl.sorted && d.n_codes > 1) {
		PolrDictSortLayout so;
		polr_dict_sort_layout(d.n_codes, &so);
		HIPCHK(ctx, sort_mem.alloc(so.total));
		DictRec *from = (DictRec *)(sort_mem + so.ping), *to = (DictRec *)(sort_mem + so.pong);
		uint4 *rep_old = (uint4 *)(sort_mem + so.rep_old);
		uint32_t *rank_of = (uint32_t *)(sort_mem + so.rank);
		hipLaunchKernelGGL(polr_dict_sort_keys_kernel, dim3((d.n_codes + 255) / 256), dim3(256), 0, st, cells, (const uint32_t *)row_of_code,
		                   d.n_codes, rep_old, from);
		hipLaunchKernelGGL(polr_dict_sort_tile_kernel, dim3(so.n_tiles), dim3(POLR_DICT_BLOCK), 0, st, from, d.n_codes,
		                   (const uint4 *)rep_old);
		for (uint32_t p = 0; p < so.n_merge_passes; p++) {
			hipLaunchKernelGGL(polr_dict_sort_merge_kernel, dim3(so.n_tiles), dim3(POLR_DICT_BLOCK), 0, st, (const DictRec *)from, to,
			                   d.n_codes, POLR_DICT_SORT_TILE << p, (const uint4 *)rep_old);
			std::swap(from, to);
		}
		hipLaunchKernelGGL(polr_dict_renumber_kernel, dim3((d.n_codes + 255) / 256), dim3(256), 0, st, (const DictRec *)from,
		                   (const uint4 *)rep_old, d.n_codes, d.cells.get(), rank_of);
		rank = rank_of;
	} else if (d.n_codes) {
		hipLaunchKernelGGL(polr_dict_reps_kernel, dim3((d.n_codes + 255) / 256), dim3(256), 0, st, cells, (const uint32_t *)row_of_code,
		                   d.n_codes, d.cells.get());
	}
	// assign (sorted codes: once their ranks are known)
	if (pl.sorted && n) {
		hipLaunchKernelGGL(polr_dict_assign_kernel, dim3(dict_grid(n, ctx->n_cus)), dim3(256), 0, st, t, (const uint32_t *)slot_of_row, n,
		                   (const uint32_t *)scalars, rank, (uint32_t *)codes.data);
	}
	if (d.n_codes || pl.sorted) {
		HIPCHK(ctx, hipStreamSynchronize(st));
	}
	return POLR_OK;
}

extern "C" int polr_ht_encode_dictionary(polr_ht *ht, uint32_t payload_col, void *stream, uint32_t *code_col, uint32_t *n_codes,
                                         uint32_t *has_null) {
	return polr_ht_encode_dictionary_ex(ht, payload_col, 0u, stream, code_col, n_codes, has_null);
}

extern "C" int polr_ht_encode_dictionary_ex(polr_ht *ht, uint32_t payload_col, uint32_t flags, void *stream, uint32_t *code_col,
                                            uint32_t *n_codes, uint32_t *has_null) {
	POLR_ENTRY();
	if (!ht || !code_col || !n_codes || !has_null) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = ht->ctx;
	// the request, and what the plan says to it
	const DictCol *prior = polr_dict_of_src_col(ht, payload_col);
	PolrDictRequest rq = {};
	rq.flags = flags;
	rq.payload_col = payload_col;
	rq.finalized = ht->kind != KIND_NONE;
	rq.n_payload = ht->n_payload;
	rq.width = payload_col < ht->n_payload ? ht->payload[payload_col].width : 0;
	rq.encoded = prior != nullptr;
	rq.encoded_as = prior ? prior->code_col : 0;
	rq.n_rows = ht->n_rows_in;
	PolrDictPlan pl;
	POLR_TRY_PLAN(ctx, pl, polr_dict_plan_encode(rq, &pl));
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	if (st != ctx->stream) {
		// (the column's cells were uploaded, and rebased onto their heap, on the context's stream)
		HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	}
	// everything up to the commit lives in this scope: a failure frees it and leaves the table exactly as it was
	const DictJob job = {&pl, &ht->payload[payload_col], rq.n_rows, nullptr, rq.n_rows, payload_col, false};
	OwnedCol codes;
	DictCol d;
	d.src_col = payload_col;
	d.code_col = ht->n_payload;
	POLR_TRY(dict_encode(ctx, st, job, codes, d));
	// commit: nothing can fail from here on.  The code column is an ordinary payload column: 4 bytes, unsigned, no validity
	// array but the one POLR_DICT_NULL_INVALID copied
	*code_col = d.code_col;
	*n_codes = d.n_codes;
	*has_null = d.has_null;
	ht->device_bytes += polr_dict_device_bytes(rq.n_rows, codes.valid != nullptr, d.n_codes);
	ht->payload.push_back(std::move(codes));
	ht->n_payload++;
	ht->dicts.push_back(std::move(d));
	return POLR_OK;
}

// Appends the code column to the pipeline's probe columns.  Pointers into polr_pipeline::probe_cols live inside one call
// only (OutCol::col, polr_out_describe_col: resolved and dropped by every sink call; the scan and the statistics likewise),
// and the device never reads the column descriptors of an output or a multiplexer through the pipeline -- their sinks hold
// DevCol copies -- so handles made before the call run on as they did.  The new descriptors are built aside and swapped in
// at the commit.
extern "C" int polr_pipeline_encode_dictionary(polr_pipeline *p, uint32_t probe_col, uint32_t flags, void *stream, uint32_t *code_col,
                                               uint32_t *n_codes, uint32_t *has_null) {
	POLR_ENTRY();
	if (!p || !code_col || !n_codes || !has_null) {
		return POLR_E_INVALID;
	}
	polr_ctx *ctx = p->ctx;
	// the request, and what the plan says to it
	const DictCol *prior = polr_dict_of_src_col(p->dicts, probe_col);
	PolrPDictRequest rq = {};
	rq.flags = flags;
	rq.probe_col = probe_col;
	rq.n_probe_cols = p->n_probe_cols;
	rq.width = probe_col < p->n_probe_cols ? p->probe_cols[probe_col].width : 0;
	rq.encoded = prior != nullptr;
	rq.encoded_as = prior ? prior->code_col : 0;
	rq.is_code_col = polr_dict_of_code_col(p->dicts, probe_col) != nullptr;
	rq.n_rows = p->n_probe_rows;
	rq.has_selection = p->sel_dev != nullptr; // (the selection in force: what POLR_STATS_SELECTED reads)
	rq.n_selected = p->n_tuples;
	PolrPDictPlan pl;
	POLR_TRY_PLAN(ctx, pl, polr_pdict_plan_encode(rq, &pl));
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	if (st != ctx->stream) {
		// (the column's cells were uploaded, and rebased onto their heap, on the context's stream)
		HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	}
	// (room for the commit's two appends first: moving the records changes nothing a caller can see)
	p->probe_cols.reserve((size_t)p->n_probe_cols + 1);
	p->dicts.reserve(p->dicts.size() + 1);
	// everything up to the commit lives in this scope: a failure frees it and leaves the pipeline exactly as it was
	const DictJob job = {&pl, &p->probe_cols[probe_col], rq.n_rows, pl.selected ? p->sel_dev : nullptr, pl.n_insert, probe_col, true};
	OwnedCol codes;
	DictCol d;
	d.src_col = probe_col;
	d.code_col = p->n_probe_cols;
	POLR_TRY(dict_encode(ctx, st, job, codes, d));
	// the descriptors with one more column: the device array of the probe columns and both variants of the pipeline
	std::vector<DevCol> cols((size_t)p->n_probe_cols + 1);
	for (uint32_t c = 0; c < p->n_probe_cols; c++) {
		cols[c] = dev_col(p->probe_cols[c]);
	}
	cols[p->n_probe_cols] = dev_col(codes);
	DevBuf<DevCol> cols_dev;
	DevBuf<DevPipeline> dev_mat, dev_count;
	HIPCHK(ctx, cols_dev.alloc(cols.size()));
	HIPCHK(ctx, dev_mat.alloc(1));
	HIPCHK(ctx, dev_count.alloc(1));
	DevPipeline host_mat = p->host_mat, host_count = p->host_count;
	host_mat.n_probe_cols = host_count.n_probe_cols = p->n_probe_cols + 1;
	host_mat.probe_cols = host_count.probe_cols = cols_dev;
	HIPCHK(ctx, hipMemcpy(cols_dev, cols.data(), cols.size() * sizeof(DevCol), hipMemcpyHostToDevice));
	HIPCHK(ctx, hipMemcpy(dev_mat, &host_mat, sizeof(DevPipeline), hipMemcpyHostToDevice));
	HIPCHK(ctx, hipMemcpy(dev_count, &host_count, sizeof(DevPipeline), hipMemcpyHostToDevice));
	// commit: nothing can fail from here on.  The code column is an ordinary probe column: 4 bytes, unsigned
	*code_col = d.code_col;
	*n_codes = d.n_codes;
	*has_null = d.has_null;
	p->probe_cols.push_back(std::move(codes));
	p->n_probe_cols++;
	p->dicts.push_back(std::move(d));
	p->probe_cols_dev = std::move(cols_dev);
	p->host_mat = host_mat;
	p->host_count = host_count;
	p->dev_mat = std::move(dev_mat);
	p->dev_count = std::move(dev_count);
	return POLR_OK;
}

// the whole dictionary `d` (NULL: none is held) as string records; probe: the pipeline's call
static int dict_fetch(polr_ctx *ctx, const DictCol *d, bool probe, uint32_t code_col, void *stream, uint64_t *offsets,
                      uint64_t n_offsets, uint8_t *str_bytes, uint64_t str_cap, uint64_t *str_used) {
	PolrPDictPlan pl;
	POLR_TRY_PLAN(ctx, pl, probe ? polr_pdict_plan_fetch(d != nullptr, code_col, 0, nullptr, 0, &pl)
	                             : polr_dict_plan_fetch(d != nullptr, code_col, 0, nullptr, 0, &pl));
	*str_used = 0;
	if (d->n_codes == 0) {
		return POLR_OK;
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	std::vector<uint4> reps(d->n_codes); // (their first words are the lengths)
	HIPCHK(ctx, hipMemcpyAsync(reps.data(), d->cells, (size_t)d->n_codes * 16, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	std::vector<uint64_t> offs(d->n_codes); // code after code
	*str_used = polr_strrec_layout(d->n_codes, [&](uint64_t c) { return (uint64_t)reps[c].x; }, offs.data());
	const int rc = polr_fetch_str_records(ctx, st, d->cells, nullptr, d->n_codes, offs.data(), *str_used, n_offsets, nullptr, str_bytes,
	                                      str_cap);
	if (rc == POLR_E_OVERFLOW) { // (nothing was written: offsets and str_bytes are as they were)
		POLR_FAIL(ctx, POLR_E_OVERFLOW, "the dictionary has %u strings in %llu bytes, the caller made room for %llu and %llu", d->n_codes,
		          (unsigned long long)*str_used, (unsigned long long)n_offsets, (unsigned long long)str_cap);
	}
	POLR_TRY(rc);
	memcpy(offsets, offs.data(), (size_t)d->n_codes * 8);
	return POLR_OK;
}

// ... and the strings of the n listed codes
static int dict_fetch_codes(polr_ctx *ctx, const DictCol *d, bool probe, uint32_t code_col, void *stream, const uint32_t *codes,
                            uint64_t n, uint64_t *offsets, uint8_t *str_bytes, uint64_t str_cap, uint64_t *str_used) {
	PolrPDictPlan pl;
	POLR_TRY_PLAN(ctx, pl, probe ? polr_pdict_plan_fetch(d != nullptr, code_col, d ? d->n_codes : 0, codes, n, &pl)
	                             : polr_dict_plan_fetch(d != nullptr, code_col, d ? d->n_codes : 0, codes, n, &pl));
	*str_used = 0;
	if (n == 0) {
		return POLR_OK;
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = polr_stream(ctx, stream);
	const uint32_t n32 = (uint32_t)n;
	DevBuf<uint32_t> d_codes, d_lens; // (the lengths come from the device: the cells stay there)
	HIPCHK(ctx, d_codes.alloc(n));
	HIPCHK(ctx, d_lens.alloc(n));
	HIPCHK(ctx, hipMemcpyAsync(d_codes, codes, (size_t)n * 4, hipMemcpyHostToDevice, st));
	hipLaunchKernelGGL(polr_dict_lens_kernel, dim3((n32 + 255) / 256), dim3(256), 0, st, (const uint4 *)d->cells.get(),
	                   (const uint32_t *)d_codes.get(), n32, d_lens.get());
	std::vector<uint32_t> lens(n);
	HIPCHK(ctx, hipMemcpyAsync(lens.data(), d_lens, (size_t)n * 4, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	std::vector<uint64_t> offs(n); // list order, a record per duplicate
	*str_used = polr_strrec_layout(n, [&](uint64_t i) { return (uint64_t)lens[i]; }, offs.data());
	const int rc = polr_fetch_str_records(ctx, st, d->cells, d_codes, n, offs.data(), *str_used, n, nullptr, str_bytes, str_cap);
	if (rc == POLR_E_OVERFLOW) { // (nothing was written: offsets and str_bytes are as they were)
		POLR_FAIL(ctx, POLR_E_OVERFLOW, "the %llu listed strings take %llu bytes, the caller made room for %llu", (unsigned long long)n,
		          (unsigned long long)*str_used, (unsigned long long)str_cap);
	}
	POLR_TRY(rc);
	memcpy(offsets, offs.data(), (size_t)n * 8);
	return POLR_OK;
}

extern "C" int polr_ht_fetch_dictionary(polr_ht *ht, uint32_t code_col, void *stream, uint64_t *offsets, uint64_t n_offsets,
                                        uint8_t *str_bytes, uint64_t str_cap, uint64_t *str_used) {
	POLR_ENTRY();
	if (!ht || !str_used || (!offsets && n_offsets) || (!str_bytes && str_cap)) {
		return POLR_E_INVALID;
	}
	return dict_fetch(ht->ctx, polr_dict_of_code_col(ht, code_col), false, code_col, stream, offsets, n_offsets, str_bytes, str_cap,
	                  str_used);
}

extern "C" int polr_ht_fetch_dictionary_codes(polr_ht *ht, uint32_t code_col, void *stream, const uint32_t *codes, uint64_t n,
                                              uint64_t *offsets, uint8_t *str_bytes, uint64_t str_cap, uint64_t *str_used) {
	POLR_ENTRY();
	if (!ht || !str_used || (n && (!codes || !offsets)) || (!str_bytes && str_cap)) {
		return POLR_E_INVALID;
	}
	return dict_fetch_codes(ht->ctx, polr_dict_of_code_col(ht, code_col), false, code_col, stream, codes, n, offsets, str_bytes,
	                        str_cap, str_used);
}

extern "C" int polr_pipeline_fetch_dictionary(polr_pipeline *p, uint32_t code_col, void *stream, uint64_t *offsets, uint64_t n_offsets,
                                              uint8_t *str_bytes, uint64_t str_cap, uint64_t *str_used) {
	POLR_ENTRY();
	if (!p || !str_used || (!offsets && n_offsets) || (!str_bytes && str_cap)) {
		return POLR_E_INVALID;
	}
	return dict_fetch(p->ctx, polr_dict_of_code_col(p->dicts, code_col), true, code_col, stream, offsets, n_offsets, str_bytes, str_cap,
	                  str_used);
}

extern "C" int polr_pipeline_fetch_dictionary_codes(polr_pipeline *p, uint32_t code_col, void *stream, const uint32_t *codes, uint64_t n,
                                                    uint64_t *offsets, uint8_t *str_bytes, uint64_t str_cap, uint64_t *str_used) {
	POLR_ENTRY();
	if (!p || !str_used || (n && (!codes || !offsets)) || (!str_bytes && str_cap)) {
		return POLR_E_INVALID;
	}
	return dict_fetch_codes(p->ctx, polr_dict_of_code_col(p->dicts, code_col), true, code_col, stream, codes, n, offsets, str_bytes,
	                        str_cap, str_used);
}
