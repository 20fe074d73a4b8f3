// duckdb-polr_amd/csrc/polr_steal.h -- range stealing between the executors of one run: the claim / steal protocol,
// compiled for BOTH sides like polr_routing.h (the pool router on the device, polr_pool_device.h; a stand-alone host
// program for the tests, tests/steal/steal_protocol_main.cpp).
//
// Reference counterpart: the task scheduler hands a worker thread that has run dry the work of another
// (src/parallel/pipeline.cpp:145-174).  Here every executor works through its own contiguous chunk range, grant by
// grant; only an executor whose range is used up takes half of what the best-off executor has left, from the far end.
//
//   word      one 64-bit word per executor: claimed:32 | end:32, both chunk indexes.  The word says "chunks
//             [claimed, end) belong to this executor and nobody has routed them yet".  claimed == end: empty.
//   grant     `grant` consecutive chunks: what an owner takes from its word at a time, and the unit steals are cut in.
//   claim     OWNER only: compare-and-swap claimed -> min(claimed + grant, end); the owner routes [old, new).
//   steal     anybody else: the victim is the word with the largest end - claimed (lowest index on ties); the thief
//             takes s = ((end - claimed) / 2 rounded down to whole grants) chunks off the END with a compare-and-swap
//             end -> end - s, provided s >= grant (the victim has at least two grants left).  It then STORES
//             {end - s, end} into its own word and goes on claiming from there.
//   retry     a failed compare-and-swap means somebody else made progress: read again.  Every success moves chunks
//             towards "routed" or halves a remainder, so the loops end; the steal loop ends when no word has two grants
//             left.  Nobody waits for anybody.
//   ordering  relaxed (agent scope on the device): the words order nothing but themselves -- the source is read-only.
//
// Why the wholesale store is safe, and why there is no ABA.  At every moment the non-empty words describe pairwise
// disjoint pieces of the table, and a chunk only ever moves from "in a word" to "claimed by its owner", never back.
//   * A thief stores into its own word only while that word is empty.  Nobody compares-and-swaps an empty word (a steal
//     needs two grants, a claim needs one chunk), so the store cannot race with a successful compare-and-swap.
//   * A stale thief holds an old value {c, e}, c < e, of a victim's word.  While the word is not empty it changes only
//     by claimed going up or end going down, so it cannot come back to {c, e} that way.  For `end` to go up again the
//     word must be rewritten wholesale, which its owner does only after the word ran empty -- after chunk c was claimed.
//     Every later value of the word describes unclaimed chunks only, hence never contains c, hence is never {c, e}.
//   So a compare-and-swap that succeeds always acts on the piece its caller has read.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define POLR_STEAL_FN __host__ __device__ __forceinline__
#else
#define POLR_STEAL_FN inline
#endif

#if !defined(__HIPCC__)
#include <atomic>
#endif

namespace polr_steal {

#if defined(__HIPCC__)
// (a HIP translation unit: the words live in global memory and only device code touches them; both compilation passes
// see the same types)
typedef unsigned long long Word;
POLR_STEAL_FN uint64_t word_load(const Word *w) {
	return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
POLR_STEAL_FN void word_store(Word *w, uint64_t v) {
	__hip_atomic_store(w, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
POLR_STEAL_FN bool word_cas(Word *w, uint64_t expect, uint64_t desired) {
	unsigned long long e = expect;
	return __hip_atomic_compare_exchange_strong(w, &e, (unsigned long long)desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
	                                            __HIP_MEMORY_SCOPE_AGENT);
}
#else
typedef std::atomic<uint64_t> Word;
inline uint64_t word_load(const Word *w) {
	return w->load(std::memory_order_relaxed);
}
inline void word_store(Word *w, uint64_t v) {
	w->store(v, std::memory_order_relaxed);
}
inline bool word_cas(Word *w, uint64_t expect, uint64_t desired) {
	return w->compare_exchange_strong(expect, desired, std::memory_order_relaxed, std::memory_order_relaxed);
}
#endif

POLR_STEAL_FN uint64_t pack(uint32_t claimed, uint32_t end) {
	return ((uint64_t)claimed << 32) | end;
}
POLR_STEAL_FN uint32_t claimed_of(uint64_t v) {
	return (uint32_t)(v >> 32);
}
POLR_STEAL_FN uint32_t end_of(uint64_t v) {
	return (uint32_t)v;
}
// chunks nobody has routed yet
POLR_STEAL_FN uint32_t remainder_of(uint64_t v) {
	return end_of(v) > claimed_of(v) ? end_of(v) - claimed_of(v) : 0u;
}
// what a thief takes from a word with `rem` chunks left: half, in whole grants (0: fewer than two grants left, no steal)
POLR_STEAL_FN uint32_t steal_amount(uint32_t rem, uint32_t grant) {
	const uint32_t s = (rem / 2u) / grant * grant;
	return s >= grant ? s : 0u;
}
// victim choice: is (rem, idx) a better victim than (best_rem, best_idx)?  Largest remainder, lowest index on ties.
POLR_STEAL_FN bool better_victim(uint32_t rem, uint32_t idx, uint32_t best_rem, uint32_t best_idx) {
	return rem > best_rem || (rem == best_rem && idx < best_idx);
}

// OWNER: the next grant of its own word -> [*begin, *end); false: the word is empty
POLR_STEAL_FN bool claim(Word *own, uint32_t grant, uint32_t *begin, uint32_t *end) {
	while (true) {
		const uint64_t v = word_load(own);
		const uint32_t c = claimed_of(v), e = end_of(v);
		if (c >= e) {
			return false;
		}
		const uint32_t nc = e - c > grant ? c + grant : e;
		if (word_cas(own, v, pack(nc, e))) {
			*begin = c;
			*end = nc;
			return true;
		}
		// (a thief shortened the word meanwhile: again)
	}
}

// THIEF, after it has picked `victim` and read its word as `seen`: take the far half.  1: stolen -- [*begin, *end) now
// sits in words[self]; 0: the compare-and-swap lost (pick again); -1: `seen` has no two grants left.
POLR_STEAL_FN int take(Word *words, uint32_t victim, uint64_t seen, uint32_t self, uint32_t grant, uint32_t *begin,
                              uint32_t *end) {
	const uint32_t s = steal_amount(remainder_of(seen), grant);
	if (s == 0 || victim == self) {
		return -1;
	}
	const uint32_t c = claimed_of(seen), e = end_of(seen);
	if (!word_cas(&words[victim], seen, pack(c, e - s))) {
		return 0;
	}
	word_store(&words[self], pack(e - s, e)); // (own word: empty, so nobody's compare-and-swap can be in its way)
	*begin = e - s;
	*end = e;
	return 1;
}

// the victim scan, one word after the other (the device router scans lane-parallel with the same better_victim):
// the word to steal from and the value read there; false: n == 0
POLR_STEAL_FN bool pick_victim(const Word *words, uint32_t n, uint32_t self, uint32_t *victim, uint64_t *seen) {
	uint32_t best_rem = 0, best = 0xFFFFFFFFu;
	uint64_t best_v = 0;
	for (uint32_t i = 0; i < n; i++) {
		if (i == self) {
			continue;
		}
		const uint64_t v = word_load(&words[i]);
		const uint32_t rem = remainder_of(v);
		if (better_victim(rem, i, best_rem, best)) {
			best_rem = rem;
			best = i;
			best_v = v;
		}
	}
	*victim = best;
	*seen = best_v;
	return best != 0xFFFFFFFFu;
}

// THIEF: steal from whoever has most left.  true: [*begin, *end) (s chunks) now sits in words[self]; false: no word
// has two grants left (the best-off one has not, so nobody has)
POLR_STEAL_FN bool steal(Word *words, uint32_t n, uint32_t self, uint32_t grant, uint32_t *begin, uint32_t *end) {
	while (true) {
		uint32_t victim;
		uint64_t seen;
		if (!pick_victim(words, n, self, &victim, &seen)) {
			return false;
		}
		const int r = take(words, victim, seen, self, grant, begin, end);
		if (r != 0) {
			return r > 0;
		}
	}
}

} // namespace polr_steal
