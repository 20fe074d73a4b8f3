// duckdb-polr_amd/csrc/polr_flat_device.h -- the probe pipeline for FLAT join banks (device code, gfx950).
//
// A pipeline is flat when every multiplexed join (a) is keyed by ONE 4-byte column of the probe table and (b) has
// at most one build row per key (KIND_PERFECT bit table or KIND_S8 unique-key hash table) -- the star joins of
// SSB / SSB-skew and the FK -> PK joins of JOB-light -- and only counters leave the pipeline (COUNT(*) sink, or
// the exploration / ALTERNATE rounds of any sink).  Then a tuple between two joins is just its position in the
// source, the reference's RunPath (src/parallel/polar_pipeline_executor.cpp:427-538) degenerates to "AND the k
// membership tests in path order, count the survivors of every prefix" (:486-487), and the generic pipeline's
// descriptors, tuple slots and expansion machinery (polr_probe_device.h) are dead weight.  What this version does:
//
//   * stage 0 streams its key column with 16-byte loads (8 tuples per lane, 512 per wave step), the next step's
//     keys requested one step ahead;
//   * bit tables small enough live in LDS for the whole run (copied once per workgroup): a lookup there is free
//     next to the key stream (measured: 4 LDS lookups per tuple at the 5.4 TB/s streaming rate, against
//     190-350 G lookups/s for an L2-resident table, tools/micro/gather_bench.hip);
//   * between stages the survivors wait in per-wave LDS queues (what CacheJoinChunk does for 1024-row chunks,
//     polar_pipeline_executor.cpp:166-195) as 16-bit positions inside the unit (a unit is at most 65 536 tuples);
//   * the deeper stages run as ONE SWEEP: when some deeper stage has a full step, up to 512 (256 beyond two joins)
//     entries are popped from EVERY deeper queue at once, all their key gathers are issued together (8 / 4 per lane
//     and stage), then all their table lookups, then the survivors are pushed on, deepest stage first.  A wave is
//     bound by dependent memory round trips (measured: 67 % of its cycles waiting with one stage at a time), and a
//     sweep pays two of them for all stages instead of two per stage.  "Issued together" is a property of the
//     COMPILED code, not of the order of the statements: until the gather and table phases were written as
//     straight-line code (flat_sweep) every load stood under a per-element branch and waited for the one before it --
//     a sweep at K = 4 paid up to 12 round trips, not two.  tools/mlp_report.py counts the waits between the marker
//     comments of the two phases (profiles/mlp_report.txt; tests/test_mlp_report.py pins them at zero for K = 4);
//   * the k stage descriptors of the current join order sit in scalar registers (loaded when the order changes).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "polr_device.h"

#define FLAT_STEP0 512       // tuples per stage-0 step
#define FLAT_UNIT_MAX 65536u // queue entries are 16-bit positions inside the unit

// entries a sweep takes from each deeper queue: 8 per lane for pipelines of up to 4 joins, 4 per lane beyond (a sweep
// holds position + key + table word of every deeper stage in registers)
template <int K>
__device__ __host__ constexpr int flat_sweep_f() {
	return K <= 2 ? 8 : 4;
}
template <int K>
__device__ __host__ constexpr int flat_qcap() { // a queue holds < one sweep when a step pushes <= 512 more
	return 64 * flat_sweep_f<K>() - 1 + 512;
}
template <int K>
__device__ __host__ constexpr int flat_qoff(int pos) { // uint16 offset of the queue that FEEDS stage pos (pos >= 1)
	return (pos - 1) * (flat_qcap<K>() + 1);
}
template <int K>
__device__ __host__ constexpr int flat_per_wave_dwords() {
	return K <= 1 ? 0 : ((K - 1) * (flat_qcap<K>() + 1) * 2 + 3) / 4;
}

// scalar view of one stage (SGPRs; loaded from the FlatStageRec array in global memory through the scalar cache)
struct FlatStage {
	const POLR_GLOBAL uint32_t *keys;
	const POLR_GLOBAL uint8_t *valid;
	const POLR_GLOBAL uint32_t *table; // bit words or {key,row} slots in HBM
	uint32_t kind_lds;     // kind | lds_off1 << 8 (lds_off1: 1 + dword offset inside the workgroup's LDS table area, 0 = HBM)
	uint32_t a, b;         // perfect: min, range (32-bit modular); hash: slot mask (capacity <= 2^31), unused
	uint32_t out_slot;     // emitting runs: the output slot of this join's build id (1 + its index in the original order)
};

// The join-order switch: the K records of join order `path` (FlatStageRec, polr_device.h: the host wrote exactly the
// words of a FlatStage when the pipeline was created), ALL requested before the first is waited for -- 3 * K 16-byte
// granules at a wave-uniform address of constant memory, so the requests go through the scalar cache straight into
// scalar registers, with no branch between them: a position beyond the pipeline's last join reads its all-zero record
// and stays inert.  (As first written every field of every StageDesc was a vector load of its own behind `p < k` and
// `kind == KIND_PERFECT ? min : mask`, each waited for before the next: about 20 dependent round trips per switch at
// K = 4.)  tools/mlp_report.py counts the requests and the waits between the two marker comments.
template <int K>
__device__ __forceinline__ void flat_load_stages(FlatStage (&st)[K], const FlatStageRec *recs_generic, uint32_t path) {
	path = uni(path);
	asm volatile("; polr-path-switch-begin" : "+s"(path)); // (the addresses hang on the marker: no request moves in front of it)
	const POLR_CONST polr_u32x4 *src = (const POLR_CONST polr_u32x4 *)((uint64_t)recs_generic) + (size_t)path * (POLR_KMAX * 3);
	polr_u32x4 w[K][3];
#pragma unroll
	for (int p = 0; p < K; p++) {
#pragma unroll
		for (int g = 0; g < 3; g++) {
			w[p][g] = src[p * 3 + g];
		}
	}
#pragma unroll
	for (int p = 0; p < K; p++) {
		asm volatile("" ::"s"(w[p][2].x), "s"(w[p][2].y)); // (the records' last words are asked for in front of the end marker too)
	}
	asm volatile("; polr-path-switch-end" ::: "memory");
#pragma unroll
	for (int p = 0; p < K; p++) {
		st[p].keys = (const POLR_GLOBAL uint32_t *)(((uint64_t)w[p][0].y << 32) | w[p][0].x);
		st[p].valid = (const POLR_GLOBAL uint8_t *)(((uint64_t)w[p][0].w << 32) | w[p][0].z);
		st[p].table = (const POLR_GLOBAL uint32_t *)(((uint64_t)w[p][1].y << 32) | w[p][1].x);
		st[p].kind_lds = w[p][1].z;
		st[p].a = w[p][1].w;
		st[p].b = w[p][2].x;
		st[p].out_slot = w[p][2].y;
	}
}

template <int K>
struct FlatCtx {
	uint32_t k, lane;
	FlatStage st[K]; // the current join order, statically indexed (SGPRs)
	const POLR_GLOBAL uint32_t *sel;
	bool plain; // no selection vector and no validity column on a deeper stage of the current order (flat_set_plain)
	const POLR_LDS uint32_t *lds_tables; // the workgroup's LDS-resident bit tables
	POLR_LDS uint16_t *q;                // this wave's queues
	uint32_t qsize[K], cnt[K];
	uint64_t unit_begin, in_pos, in_end;
	// emitting runs (a materialising sink behind a bank of perfect tables): the final tuples as row ids, chunked like a
	// DataChunk stream -- slot 0 the probe row, slot 1 + j the build id of join j = its key's offset in the perfect table
	DevOut out;
	OutState os;
	POLR_LDS unsigned long long *fused_lds; // the workgroup's group cells of a fused GROUP BY sink, when they fit in LDS
	// stage 0's next step, requested one step ahead (the key stream's HBM round trip overlaps the current step)
	uint4 pf0, pf1;
	uint64_t pf_pos; // source position the prefetched keys belong to; ~0: none
};

// ---- membership test in two halves: issue (addresses + loads in flight), then resolve -------------------------
// perfect table: 32-bit modular arithmetic, exact for signed and unsigned 4-byte keys while [min, max] lies inside the
// key type's domain (checked on the host).  Every element loads a word, with no branch around the load: an element
// whose key is out of range reads the table's last word, and its word counts for nothing -- idx says so (an inactive
// element gets FLAT_NO_IDX, beyond every range: a table spans less than 2^31 values).  (A load under a per-element
// branch makes the compiler wait for every load before it issues the next.  The index is clamped, not chosen with a
// select, and no flag lives across the load: flags are scalar register pairs, and with them K = 4 spilled 15 VGPRs.)
#define FLAT_NO_IDX 0xFFFFFFFFu
template <int F>
__device__ __forceinline__ void flat_perfect_issue(const FlatStage &s, const POLR_LDS uint32_t *lds_tables, const uint32_t (&key)[F],
                                                   const bool (&act)[F], uint32_t (&idx)[F], uint32_t (&w)[F]) {
	const uint32_t lds_off1 = s.kind_lds >> 8;
	uint32_t at[F];
#pragma unroll
	for (int i = 0; i < F; i++) {
		idx[i] = act[i] ? key[i] - s.a : FLAT_NO_IDX;
		at[i] = (idx[i] < s.b ? idx[i] : s.b) >> 5;
	}
	// (one address space per stage, wave-uniform: DS_READ or GLOBAL_LOAD, never a generic access)
	if (lds_off1) {
		const POLR_LDS uint32_t *bits = lds_tables + (lds_off1 - 1u);
#pragma unroll
		for (int i = 0; i < F; i++) {
			w[i] = bits[at[i]];
		}
	} else {
#pragma unroll
		for (int i = 0; i < F; i++) {
			w[i] = s.table[at[i]];
		}
	}
}

// unique-key hash table: linear probing, one aligned 32-byte group of 4 {key,row} slots per round trip, four probes in
// flight per lane (eight would hold 64 VGPRs of slot data)
template <int F>
__device__ __forceinline__ void flat_hash_lookup(const FlatStage &s, const uint32_t (&key)[F], const bool (&act)[F],
                                                 bool (&hit)[F]) {
	const POLR_GLOBAL uint32_t *tab = s.table; // (groups of 8 dwords)
#pragma unroll
	for (int h0 = 0; h0 < F; h0 += 4) {
		uint32_t group[4], first[4];
		bool searching[4];
		bool any = false;
		const uint32_t gmask = s.a >> 2;
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const uint64_t h = polr_murmurhash64((uint64_t)key[h0 + i]) & (uint64_t)s.a;
			group[i] = (uint32_t)(h >> 2);
			first[i] = (uint32_t)(h & 3u);
			searching[i] = act[h0 + i];
			hit[h0 + i] = false;
			any = any || searching[i];
		}
		while (__ballot(any) != 0ull) {
			uint4 a[4], b[4];
#pragma unroll
			for (int i = 0; i < 4; i++) {
				if (searching[i]) {
					a[i] = load_global_x4(tab + (uint64_t)group[i] * 8);
					b[i] = load_global_x4(tab + (uint64_t)group[i] * 8 + 4);
				}
			}
			any = false;
#pragma unroll
			for (int i = 0; i < 4; i++) {
				if (searching[i]) {
					// (s8_group_step of polr_device.h, spelled out: called here it leaves the same result, but the flat
					// kernels' register allocation changes -- 7 more spilled SGPRs at K = 2)
					const uint32_t kk[4] = {a[i].x, a[i].z, b[i].x, b[i].z};
					const uint32_t rr[4] = {a[i].y, a[i].w, b[i].y, b[i].w};
#pragma unroll
					for (int j = 0; j < 4; j++) {
						if (searching[i] && (uint32_t)j >= first[i]) {
							if (rr[j] == S8_EMPTY_ROW) {
								searching[i] = false;
							} else if (kk[j] == key[h0 + i]) {
								hit[h0 + i] = true;
								searching[i] = false;
							}
						}
					}
					first[i] = 0;
					group[i] = (group[i] + 1) & gmask;
				}
				any = any || searching[i];
			}
		}
	}
}

template <int F>
__device__ __forceinline__ void flat_lookup(const FlatStage &s, const POLR_LDS uint32_t *lds_tables, const uint32_t (&key)[F],
                                            const bool (&act)[F], bool (&hit)[F]) {
	if ((s.kind_lds & 0xFFu) == KIND_PERFECT) {
		uint32_t idx[F], w[F];
		flat_perfect_issue<F>(s, lds_tables, key, act, idx, w);
#pragma unroll
		for (int i = 0; i < F; i++) {
			hit[i] = idx[i] <= s.b && ((w[i] >> (idx[i] & 31u)) & 1u) != 0;
		}
	} else {
		flat_hash_lookup<F>(s, key, act, hit);
	}
}

#ifndef POLR_FLAT_EMIT
#define POLR_FLAT_EMIT 0 // 1: the build whose last join can write row ids (a counting run never pays for that code:
                         // inlined at every place a stage emits it cost the SF100 headline 6 % -- 96 more spilled SGPRs)
#endif
// the fused GROUP BY sink (FusedSink, polr_device.h): slot 0 = the probe row, slot 1 + j = the build id of join j, which
// the stage that probed join j holds (id[p], out_slot = 1 + j).  One lane = one surviving tuple.
template <int K>
__device__ __forceinline__ void flat_fused_accumulate(FlatCtx<K> &c, uint32_t row) {
	const FusedSink *f = c.out.fused; // (a generic pointer: the descriptor is read a few times per surviving tuple)
	auto slot_row = [&](uint32_t slot) { // (slot is wave-uniform: one stage's key column is read, if any)
		uint32_t r = row;
#pragma unroll
		for (int p = 0; p < K; p++) {
			if (p < (int)c.k && c.st[p].out_slot == slot) {
				r = c.st[p].keys[row] - c.st[p].a;
			}
		}
		return r;
	};
	uint64_t g = 0;
	bool ok = true;
	for (uint32_t q = 0; q < f->groups.n; q++) {
		const DevGroupKey gk = f->groups.k[q];
		const uint32_t r = slot_row(gk.slot);
		if (gk.src.valid && !as_global(gk.src.valid)[r]) {
			ok = false;
			break;
		}
		const unsigned long long off = (unsigned long long)(load_col_cell(gk.src, r) - gk.min_value);
		if (off >= gk.n_values) {
			ok = false;
			break;
		}
		g = g * gk.n_values + off;
	}
	if (!ok) {
		__hip_atomic_fetch_add(f->dropped, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		return;
	}
	const uint32_t n_aggs = f->aggs.n;
	// the cells of this workgroup: in LDS when they fit (flushed when the workgroup leaves: 25 M adds to a few hundred
	// global addresses cost the SF100 run 1.9 ms), else its table in global memory; adds nobody waits for either way
	const size_t at = g * (1u + 2u * n_aggs);
	unsigned long long *gcell = f->cells + (size_t)(blockIdx.x % f->n_tables) * f->words_per_table + at;
	POLR_LDS unsigned long long *lcell = c.fused_lds + at;
	const bool in_lds = c.fused_lds != nullptr;
	auto add = [&](uint32_t w, unsigned long long v) {
		if (in_lds) {
			__hip_atomic_fetch_add(&lcell[w], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		} else {
			__hip_atomic_fetch_add(&gcell[w], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
	};
	add(0, 1ull);
	for (uint32_t a = 0; a < n_aggs; a++) {
		const DevAgg ag = f->aggs.a[a];
		if (ag.fn == POLR_DEV_AGG_COUNT_STAR) {
			continue; // (= the rows of the group)
		}
		const uint32_t r = slot_row(ag.slot);
		if (ag.src.valid) {
			if (!as_global(ag.src.valid)[r]) {
				continue;
			}
			add(2u + 2u * a, 1ull);
		}
		if (ag.fn == POLR_DEV_AGG_SUM) {
			add(1u + 2u * a, (unsigned long long)load_col_cell(ag.src, r));
		}
	}
}

// the tuples that survived the last join leave as row ids (emitting runs): the probe row, and for every join the build id
// its key stands for -- every join of an emitting flat pipeline is a perfect table, whose build id IS key - min
// (RowOperations::Gather reads payload columns re-ordered that way: polr_gather.hip) -- re-read from the probe columns
// for the few tuples that get this far
template <int K>
__device__ __forceinline__ void flat_out_write(FlatCtx<K> &c, uint32_t pos, bool valid) {
	const uint64_t m = __ballot(valid);
	const uint32_t n = (uint32_t)__popcll(m);
	if (n == 0) {
		return;
	}
	POLR_GLOBAL uint32_t *ids = as_global(c.out.ids);
	uint32_t row = 0, id[K];
	if (valid) {
		const uint64_t tp = c.unit_begin + pos;
		row = c.sel ? c.sel[tp] : (uint32_t)tp;
	}
	if (c.out.fused) {
		// a fused GROUP BY sink: the tuple is folded into the group cells of its workgroup, nothing is written (and only
		// the build ids the sink's columns hang on are re-read)
		if (valid) {
			flat_fused_accumulate<K>(c, row);
		}
		return;
	}
	if (valid) {
#pragma unroll
		for (int p = 0; p < K; p++) {
			id[p] = p < (int)c.k ? c.st[p].keys[row] - c.st[p].a : 0u;
		}
	}
	out_claim(c.out, c.os, c.lane, m, valid, [&](uint64_t place) {
		ids[place] = row;
#pragma unroll
		for (int p = 0; p < K; p++) {
			if (p < (int)c.k) {
				ids[(uint64_t)c.st[p].out_slot * c.out.slot_stride + place] = id[p];
			}
		}
	});
}

// survivors of stage POS: count them; push their unit positions to the next stage's queue unless POS is the last join
template <int K, int POS, int F>
__device__ __forceinline__ void flat_emit(FlatCtx<K> &c, const uint32_t (&pos)[F], const bool (&hit)[F]) {
	const bool last = POS + 1 >= K || POS + 1 == (int)c.k;
	uint32_t total = 0;
#if POLR_FLAT_EMIT
	if (last && c.os.emit) {
		// (ONE copy of the sink's code per place a stage emits, not F: the loop stays a loop -- the element is picked
		// with selects -- or the emitting build is 2.4 ms where the counting build is 1.5)
#pragma unroll 1
		for (int i = 0; i < F; i++) {
			uint32_t p_i = pos[0];
			bool h_i = hit[0];
#pragma unroll
			for (int j = 1; j < F; j++) {
				p_i = j == i ? pos[j] : p_i;
				h_i = j == i ? hit[j] : h_i;
			}
			flat_out_write<K>(c, p_i, h_i);
		}
	}
#endif
	if constexpr (POS + 1 < K) {
		POLR_LDS uint16_t *qq = c.q + flat_qoff<K>(POS + 1);
		uint32_t qs = c.qsize[POS + 1];
#pragma unroll
		for (int i = 0; i < F; i++) {
			const uint64_t m = __ballot(hit[i]);
			const uint32_t n = (uint32_t)__popcll(m);
			if (!last && hit[i]) {
				qq[qs + lane_rank(m)] = (uint16_t)pos[i];
			}
			qs += n;
			total += n;
		}
		if (!last) {
			c.qsize[POS + 1] = qs;
		}
	} else {
#pragma unroll
		for (int i = 0; i < F; i++) {
			total += (uint32_t)__popcll(__ballot(hit[i]));
		}
	}
	c.cnt[POS] += total;
}

// one step of stage 0: up to 512 tuples straight from the source, looked up and pushed on in two halves of 256 (four
// keys per lane live at a time: the step's registers are its 8 keys + the 8 prefetched ones)
template <int K>
__device__ __forceinline__ void flat_stage0(FlatCtx<K> &c) {
	constexpr int F = 4;
	const FlatStage &s = c.st[0];
	const uint64_t left = c.in_end - c.in_pos;
	const uint32_t n = left < FLAT_STEP0 ? (uint32_t)left : (uint32_t)FLAT_STEP0;
	const uint32_t upos = (uint32_t)(c.in_pos - c.unit_begin); // position of the step inside the unit
	const bool streamable = c.sel == nullptr && s.valid == nullptr && (c.in_pos & 3ull) == 0 && (((uint64_t)s.keys) & 15ull) == 0;
	if (n == FLAT_STEP0 && streamable) {
		// lane l holds tuples in_pos + 256 h + 4 l + {0..3}: two 16-byte loads per lane
		const uint32_t base = (uint32_t)c.in_pos + 4u * c.lane;
		uint4 kk[2];
		if (c.pf_pos == c.in_pos) {
			kk[0] = c.pf0;
			kk[1] = c.pf1;
		} else {
			kk[0] = load_global_x4(s.keys + base);
			kk[1] = load_global_x4(s.keys + base + 256u);
		}
		if (c.in_end - c.in_pos >= 2ull * FLAT_STEP0) {
			c.pf0 = load_global_x4(s.keys + base + FLAT_STEP0);
			c.pf1 = load_global_x4(s.keys + base + FLAT_STEP0 + 256u);
			c.pf_pos = c.in_pos + FLAT_STEP0;
		} else {
			c.pf_pos = ~0ull;
		}
		c.in_pos += n;
#pragma unroll
		for (int h = 0; h < 2; h++) {
			const uint32_t key[F] = {kk[h].x, kk[h].y, kk[h].z, kk[h].w};
			uint32_t pos[F];
			bool act[F], hit[F];
#pragma unroll
			for (int i = 0; i < F; i++) {
				pos[i] = upos + 4u * c.lane + h * 256u + i;
				act[i] = true;
			}
			flat_lookup<F>(s, c.lds_tables, key, act, hit);
			flat_emit<K, 0, F>(c, pos, hit);
		}
		return;
	}
	// the lane-per-tuple step: 256 tuples at a time in (up to) two batches of loads -- the rows of a selection vector,
	// then keys and validity bytes together.  No load stands under a per-element branch: a slot past the end of the
	// step reads what the step's first tuple reads and stays inactive; a stage without validity column reads byte 0 of
	// its key column for every slot, and the byte counts for nothing.
	c.pf_pos = ~0ull;
	const uint64_t pos0 = c.in_pos;
	c.in_pos += n;
	const bool has_valid = s.valid != nullptr;
	const POLR_GLOBAL uint8_t *vbytes = has_valid ? s.valid : (const POLR_GLOBAL uint8_t *)s.keys;
	const uint32_t vmask = has_valid ? 0xFFFFFFFFu : 0u;
	const uint32_t no_valid = has_valid ? 0u : 1u; // (every byte is looked at either way: no load is left unwaited)
#pragma unroll 1
	for (uint32_t h = 0; h * 256u < n; h++) {
		uint32_t pos[F], row[F], key[F], vb[F];
		bool act[F], hit[F];
		asm volatile("; polr-stage0-slow-begin" ::: "memory");
#pragma unroll
		for (int i = 0; i < F; i++) {
			const uint32_t off = h * 256u + c.lane + 64u * i;
			act[i] = off < n;
			pos[i] = upos + off;
			row[i] = act[i] ? off : 0u; // (still the offset inside the step)
		}
		if (c.sel) {
#pragma unroll
			for (int i = 0; i < F; i++) {
				row[i] = c.sel[pos0 + row[i]];
			}
			__builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0): one wait for the batch, not one in front of every key's load
		} else {
#pragma unroll
			for (int i = 0; i < F; i++) {
				row[i] += (uint32_t)pos0;
			}
		}
#pragma unroll
		for (int i = 0; i < F; i++) {
			key[i] = s.keys[row[i]];
			vb[i] = vbytes[row[i] & vmask];
		}
		asm volatile("; polr-stage0-slow-end" ::: "memory");
#pragma unroll
		for (int i = 0; i < F; i++) {
			act[i] = act[i] && (vb[i] | no_valid) != 0; // NULL never matches (join_hashtable.cpp:170-192)
		}
		flat_lookup<F>(s, c.lds_tables, key, act, hit);
		flat_emit<K, 0, F>(c, pos, hit);
	}
}

// ---- the sweep over the deeper stages ------------------------------------------------------------------------------
template <int I, int N, class Fn>
__device__ __forceinline__ void flat_static_for(Fn &&fn) {
	if constexpr (I < N) {
		fn(std::integral_constant<int, I> {});
		flat_static_for<I + 1, N>(fn);
	}
}
template <int I, int N, class Fn>
__device__ __forceinline__ void flat_static_for_down(Fn &&fn) { // I = N-1 ... 1
	if constexpr (I >= 1) {
		fn(std::integral_constant<int, I> {});
		flat_static_for_down<I - 1, N>(fn);
	}
}

#define FLAT_INACTIVE 0xFFFFFFFFu // the position of a sweep slot that holds no tuple (no unit position is that large)

// take up to one sweep from the queue that feeds stage P.  Every slot reads the queue -- a slot beyond the entries taken
// reads the first one taken (an allocated entry even when the queue is empty) and becomes FLAT_INACTIVE: no branch
// stands around a read
template <int K, int P, int F>
__device__ __forceinline__ void flat_pop(FlatCtx<K> &c, uint32_t (&pos)[F]) {
	const uint32_t qs = c.qsize[P];
	const uint32_t n = qs < (uint32_t)(64 * F) ? qs : (uint32_t)(64 * F);
	const uint32_t base = qs - n;
	const POLR_LDS uint16_t *qq = c.q + flat_qoff<K>(P);
#pragma unroll
	for (int i = 0; i < F; i++) {
		const uint32_t off = c.lane + 64u * i;
		const uint32_t e = qq[base + (off < n ? off : 0u)];
		pos[i] = off < n ? e : FLAT_INACTIVE;
	}
	c.qsize[P] = base;
}

// the values are in their registers when this point is reached: loads that write them have come back
template <int F>
__device__ __forceinline__ void flat_await(const uint32_t (&v)[F]) {
	static_assert(F == 4 || F == 8, "sweep widths");
	if constexpr (F == 4) {
		asm volatile("; polr-sweep-await" ::"v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]));
	} else {
		asm volatile("; polr-sweep-await" ::"v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7]));
	}
}

// All deeper stages at once.  Per stage two registers per tuple live across the memory round trips: its position in
// the unit (from phase 2 on with the bit to test in its upper half) and its key, later the table word (hash stages:
// the hit flag).  (With a third register for the bit, K = 6 and K = 8 spill inside the two phases.)
//   1. pop up to one sweep from EVERY deeper queue and request the keys    -> all key gathers in flight together
//   2. bit-table stages: request the bit words                             -> all table loads in flight together
//      hash stages: probe
//   3. push the survivors on, deepest stage first (the queue a stage pushes into has just been popped: it has room)
// "In flight together" has to be written, it does not follow from the order of the statements: a load under a
// per-element branch (`if (active) key = keys[row]`) or a wave-uniform branch between two loads makes the compiler
// wait for ALL loads in flight (s_waitcnt vmcnt(0)) before the next one -- the sweep as first written paid one round
// trip per load, up to 12 at K = 4.  So phases 1 and 2 are straight-line code:
//   * every slot loads.  An inactive slot (FLAT_INACTIVE: beyond the queue's entries, NULL key, key outside the table's
//     range) reads what the unit's FIRST tuple reads -- a row of the same column, one request for all such lanes -- or
//     some word of the table, and the value counts for nothing: it never counts, pushes or emits (phase 3 asks the
//     position);
//   * a stage beyond the pipeline's last join (k < K) has an empty queue: all its slots are inactive, it reads stage 0's
//     key column;
//   * whether there is a selection vector or a validity column is decided ONCE per sweep (c.plain), not per stage.
// The marker comments are read by tools/mlp_report.py, which counts loads and waits between them.
template <int K>
__device__ __forceinline__ void flat_sweep(FlatCtx<K> &c) {
	constexpr int F = flat_sweep_f<K>();
	if constexpr (K > 1) {
		// pos: the position in the unit (bits 0-15; after phase 2 the bit to test in bits 16-20), FLAT_INACTIVE when the slot
		// is out of the running; key: the key, after phase 2 the table word (hash stages: the hit flag)
		uint32_t pos[K - 1][F], key[K - 1][F];
		if (c.plain) {
			asm volatile("; polr-sweep-keys-begin" ::: "memory");
			flat_static_for<1, K>([&](auto P) {
				constexpr int p = decltype(P)::value;
				// (the unit's rows as a scalar base + a 16-bit position: one address register per gather)
				const POLR_GLOBAL uint32_t *keys = (p < (int)c.k ? c.st[p].keys : c.st[0].keys) + (uint32_t)c.unit_begin;
				flat_pop<K, p, F>(c, pos[p - 1]);
#pragma unroll
				for (int i = 0; i < F; i++) {
					key[p - 1][i] = keys[pos[p - 1][i] != FLAT_INACTIVE ? pos[p - 1][i] : 0u];
				}
			});
			asm volatile("; polr-sweep-keys-end" ::: "memory");
		} else {
			// two batches: the rows (a selection vector's entries), ONE wait, then keys and validity bytes together (a stage
			// without validity column reads byte 0 of its key column for every slot)
			uint32_t vb[K - 1][F];
			asm volatile("; polr-sweep-sel-keys-begin" ::: "memory");
			flat_static_for<1, K>([&](auto P) {
				constexpr int p = decltype(P)::value;
				flat_pop<K, p, F>(c, pos[p - 1]);
#pragma unroll
				for (int i = 0; i < F; i++) {
					key[p - 1][i] = pos[p - 1][i] != FLAT_INACTIVE ? pos[p - 1][i] : 0u; // (the row, from here to its key's load)
				}
			});
			if (c.sel) {
				flat_static_for<1, K>([&](auto P) {
					constexpr int p = decltype(P)::value;
#pragma unroll
					for (int i = 0; i < F; i++) {
						key[p - 1][i] = c.sel[c.unit_begin + key[p - 1][i]];
					}
				});
				__builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0): the one wait, here and not load by load further down
			} else {
				flat_static_for<1, K>([&](auto P) {
					constexpr int p = decltype(P)::value;
#pragma unroll
					for (int i = 0; i < F; i++) {
						key[p - 1][i] += (uint32_t)c.unit_begin;
					}
				});
			}
			flat_static_for<1, K>([&](auto P) {
				constexpr int p = decltype(P)::value;
				const bool live = p < (int)c.k;
				const POLR_GLOBAL uint32_t *keys = live ? c.st[p].keys : c.st[0].keys;
				const bool has_valid = live && c.st[p].valid != nullptr;
				const POLR_GLOBAL uint8_t *vbytes = has_valid ? c.st[p].valid : (const POLR_GLOBAL uint8_t *)keys;
				const uint32_t vmask = has_valid ? 0xFFFFFFFFu : 0u;
#pragma unroll
				for (int i = 0; i < F; i++) {
					const uint32_t row = key[p - 1][i];
					vb[p - 1][i] = vbytes[row & vmask];
					key[p - 1][i] = keys[row];
				}
			});
			asm volatile("; polr-sweep-sel-keys-end" ::: "memory");
			__builtin_amdgcn_sched_barrier(0); // (what looks at the bytes stays behind the batch: its first wait is not part of it)
			flat_static_for<1, K>([&](auto P) {
				constexpr int p = decltype(P)::value;
				// (every byte is looked at, with or without validity column: a load nobody waits for would be waited for at
				// the next sweep's first register write -- with the source's prefetch, which that wait would force home)
				const uint32_t no_valid = p < (int)c.k && c.st[p].valid != nullptr ? 0u : 1u;
#pragma unroll
				for (int i = 0; i < F; i++) {
					pos[p - 1][i] = (vb[p - 1][i] | no_valid) != 0 ? pos[p - 1][i] : FLAT_INACTIVE; // NULL never matches
				}
			});
		}
		flat_static_for<1, K>([&](auto P) { flat_await<F>(key[decltype(P)::value - 1]); });
		asm volatile("; polr-sweep-tables-begin" ::: "memory");
		flat_static_for<1, K>([&](auto P) {
			constexpr int p = decltype(P)::value;
			if (p < (int)c.k && (c.st[p].kind_lds & 0xFFu) == KIND_PERFECT) {
				const FlatStage &s = c.st[p];
				const uint32_t lds_off1 = s.kind_lds >> 8;
				uint32_t at[F];
#pragma unroll
				for (int i = 0; i < F; i++) {
					const uint32_t idx = key[p - 1][i] - s.a;
					const bool in = pos[p - 1][i] != FLAT_INACTIVE && idx <= s.b;
					// (the bit to test rides in the position's upper half: two registers per tuple wait for the word, not three)
					pos[p - 1][i] = in ? pos[p - 1][i] | ((idx & 31u) << 16) : FLAT_INACTIVE;
					at[i] = (idx < s.b ? idx : s.b) >> 5; // (out of range: the table's last word, for nothing)
				}
				// (one address space per stage, wave-uniform: DS_READ or GLOBAL_LOAD, never a generic access)
				if (lds_off1) {
					const POLR_LDS uint32_t *bits = c.lds_tables + (lds_off1 - 1u);
#pragma unroll
					for (int i = 0; i < F; i++) {
						key[p - 1][i] = bits[at[i]];
					}
				} else {
#pragma unroll
					for (int i = 0; i < F; i++) {
						key[p - 1][i] = s.table[at[i]];
					}
				}
			}
		});
		asm volatile("; polr-sweep-tables-end" ::: "memory");
		flat_static_for<1, K>([&](auto P) {
			constexpr int p = decltype(P)::value;
			if (p < (int)c.k && (c.st[p].kind_lds & 0xFFu) != KIND_PERFECT) {
				bool act[F], hit[F];
#pragma unroll
				for (int i = 0; i < F; i++) {
					act[i] = pos[p - 1][i] != FLAT_INACTIVE;
				}
				flat_hash_lookup<F>(c.st[p], key[p - 1], act, hit);
#pragma unroll
				for (int i = 0; i < F; i++) {
					key[p - 1][i] = hit[i] ? 1u : 0u; // (bit 0: the position's upper half is 0)
				}
			}
		});
		flat_static_for_down<K - 1, K>([&](auto P) {
			constexpr int p = decltype(P)::value;
			if (p < (int)c.k) {
				bool hit[F];
#pragma unroll
				for (int i = 0; i < F; i++) {
					hit[i] = pos[p - 1][i] != FLAT_INACTIVE && ((key[p - 1][i] >> ((pos[p - 1][i] >> 16) & 31u)) & 1u) != 0;
					pos[p - 1][i] &= 0xFFFFu;
				}
				flat_emit<K, p, F>(c, pos[p - 1], hit);
			}
		});
	}
}

// whether a sweep takes its straight path: no selection vector, and no deeper stage of the current join order reads a
// validity column (set when the join order changes)
template <int K>
__device__ __forceinline__ void flat_set_plain(FlatCtx<K> &c) {
	bool plain = c.sel == nullptr;
#pragma unroll
	for (int p = 1; p < K; p++) {
		plain = plain && !(p < (int)c.k && c.st[p].valid != nullptr);
	}
	c.plain = plain;
}

// One unit [in_pos, in_end) in two phases, so that the caller can look for its next unit in between:
//   flat_run_source -- a sweep whenever a deeper stage holds a full step, else the source, until the source is used up;
//   flat_run_drain  -- sweeps until every queue is empty (a unit leaves nothing behind: its counters are final when it
//                      arrives).
// (Measured and dropped: sending a small unit, or the queue remainders at the end of a unit, down ALL remaining stages
// at once -- two round trips instead of two per stage, but keys and table words are then loaded for tuples that are
// already dead, and on a device whose memory system is the bottleneck that costs more than the chain it saves: SF100
// run 1.58 -> 1.77 ms.)
template <int K>
__device__ __forceinline__ void flat_run_source(FlatCtx<K> &c) {
	while (true) {
		bool deep_full = false;
#pragma unroll
		for (int p = 1; p < K; p++) {
			if (p < (int)c.k) {
				deep_full = deep_full || c.qsize[p] >= (uint32_t)(64 * flat_sweep_f<K>());
			}
		}
		if (deep_full) {
			flat_sweep<K>(c);
		} else if (c.in_pos < c.in_end) {
			flat_stage0<K>(c);
		} else {
			return;
		}
	}
}

template <int K>
__device__ __forceinline__ void flat_run_drain(FlatCtx<K> &c) {
	while (true) {
		bool deep_any = false;
#pragma unroll
		for (int p = 1; p < K; p++) {
			if (p < (int)c.k) {
				deep_any = deep_any || c.qsize[p] > 0;
			}
		}
		if (!deep_any) {
			return;
		}
		flat_sweep<K>(c);
	}
}

// the first source step of the unit AFTER the current one, requested while the current one drains (same join order,
// streamable source): flat_stage0 finds the keys in pf0 / pf1 when that unit starts
template <int K>
__device__ __forceinline__ void flat_prefetch_unit(FlatCtx<K> &c, uint64_t begin, uint32_t count) {
	const FlatStage &s = c.st[0];
	const bool streamable = c.sel == nullptr && s.valid == nullptr && (begin & 3ull) == 0 && (((uint64_t)s.keys) & 15ull) == 0;
	if (count >= (uint32_t)FLAT_STEP0 && streamable) {
		const uint32_t base = (uint32_t)begin + 4u * c.lane;
		c.pf0 = load_global_x4(s.keys + base);
		c.pf1 = load_global_x4(s.keys + base + 256u);
		c.pf_pos = begin;
	}
}
