// duckdb-polr_amd/csrc/polr_strcopy.h -- copy the bytes of one heap string into a packed output heap, and where a row's
// bytes go in that heap.  Defined once for host and device (as polr_strcmp.h and polr_like.h are).
//
// Reference: RowOperations::Gather for string_t (src/common/row_operations/row_gather.cpp:47-86) hands every long string
// of the result its own bytes in the result vector's heap.  polr_out_materialize_strings (polr_strout.hip) does the same
// for the output rows of a pipeline: the heap is PACKED -- row i's bytes start at the sum of the lengths of the non-NULL
// rows before it that are longer than 12 bytes (polr_str_heap_bytes), 64-bit throughout -- so source and destination of
// a copy are both unaligned, and their alignments differ.
//
// polr_str_copy(dst, src, len, lane, n_lanes): lane `lane` of `n_lanes` lanes that copy ONE string together; n_lanes = 1
// is a lane copying alone.  The destination is cut at its own 8-byte boundaries:
//   head   the bytes before the first aligned word (0-7; all of a string that ends before it)       lane 0
//   body   whole aligned words, one 8-byte store each; word k belongs to lane k mod n_lanes           every lane
//   tail   the bytes behind the last whole word (0-7)                                                 lane 1 (0 when alone)
// Reads follow the rule of polr_like.h: only the aligned 8-byte words that contain bytes of the string are loaded, so
// nothing outside [src, src + len) rounded to those words is touched.  A body word whose source straddles two aligned
// words is put together from both with shifts; the second of them always holds a byte of the string (the eight bytes
// wanted end in it).  The head's bytes are the low bytes of the string's first eight, the tail's the high bytes of its last
// eight (a heap string has more than 12), so each edge costs one or two loads and no byte is fetched singly.
// Writes touch ONLY the bytes dst[0 .. len): head and tail are written with one byte store and half-word stores at
// 2-aligned addresses -- never a wider store that would have to carry a neighbour's bytes, because in a packed heap
// those belong to another lane's string (no read-modify-write of a destination word anywhere).
// Loads come before stores.  A load issued behind a store waits for that store too (the memory counter counts both), so a
// lane copying alone takes four destination words a step: the four or five aligned source words first (and, in the first
// step, the edges' words), then all the stores -- a 20-40-byte string is one step, one wait.
// With 64 lanes a step of the body moves 512 contiguous bytes per wave: a string of n bytes takes n / 512 steps instead of
// the n / 32 of one lane.
//
// tests/test_strcopy.py runs this file in a host program (tests/strcopy/strcopy_main.cpp), plain and under the address +
// undefined-behaviour sanitizers: every source alignment x destination alignment, source allocations of exactly the
// words the rule allows, destinations between canaries.
#pragma once

#include <stdint.h>

#include "polr_strcmp.h"

// The longest string one lane copies alone in the write pass of polr_out_materialize_strings; a longer one is copied by
// the whole wave, lanes striding over its words.  Chosen by measurement: profiles/README.md, "String output".
#ifndef POLR_STRCOPY_LANE_MAX
#define POLR_STRCOPY_LANE_MAX 128u
#endif

// the heap bytes a row takes: NULL rows and inline strings take none
POLR_STRCMP_HD uint64_t polr_str_heap_bytes(uint32_t len, bool valid) {
	return valid && len > 12u ? (uint64_t)len : 0ull;
}

// offsets[i] = where row i's bytes start in the packed heap (the exclusive 64-bit prefix of polr_str_heap_bytes);
// returns the heap's size.  The host form of what the measuring pass computes with a scan.
static inline uint64_t polr_str_pack_offsets(const uint32_t *lens, const uint8_t *valid, uint64_t n, uint64_t *offsets) {
	uint64_t at = 0;
	for (uint64_t i = 0; i < n; i++) {
		offsets[i] = at;
		at += polr_str_heap_bytes(lens[i], valid ? valid[i] != 0 : true);
	}
	return at;
}

// the eight bytes [s, s + 8), all of them inside the string: put together from the one or two aligned words that hold them
// (both hold bytes of the string, so the read rule above is kept)
POLR_STRCMP_HD uint64_t polr_strcopy_load8(uint64_t s) {
	const uint64_t a = s & ~7ull;
	const uint32_t shift = 8u * (uint32_t)(s & 7ull);
	uint64_t w = *(const POLR_STRCMP_MEM uint64_t *)a;
	if (shift) {
		w = (w >> shift) | (*(const POLR_STRCMP_MEM uint64_t *)(a + 8ull) << (64u - shift));
	}
	return w;
}

// the n low bytes of v (n = 1 .. 7) to d, where d + n is 8-aligned (the head of a string): a byte, then half-words
POLR_STRCMP_HD void polr_strcopy_store_head(uint64_t d, uint64_t v, uint32_t n) {
	if (n & 1u) {
		*(POLR_STRCMP_MEM uint8_t *)d = (uint8_t)v;
		d += 1ull;
		v >>= 8;
	}
	if (n & 2u) {
		*(POLR_STRCMP_MEM uint16_t *)d = (uint16_t)v;
		d += 2ull;
		v >>= 16;
	}
	if (n & 4u) {
		*(POLR_STRCMP_MEM uint16_t *)d = (uint16_t)v;
		*(POLR_STRCMP_MEM uint16_t *)(d + 2ull) = (uint16_t)(v >> 16);
	}
}

// the n low bytes of v (n = 1 .. 7) to the 8-aligned address d (the tail of a string): half-words, then a byte
POLR_STRCMP_HD void polr_strcopy_store_tail(uint64_t d, uint64_t v, uint32_t n) {
	if (n & 4u) {
		*(POLR_STRCMP_MEM uint16_t *)d = (uint16_t)v;
		*(POLR_STRCMP_MEM uint16_t *)(d + 2ull) = (uint16_t)(v >> 16);
		d += 4ull;
		v >>= 32;
	}
	if (n & 2u) {
		*(POLR_STRCMP_MEM uint16_t *)d = (uint16_t)v;
		d += 2ull;
		v >>= 16;
	}
	if (n & 1u) {
		*(POLR_STRCMP_MEM uint8_t *)d = (uint8_t)v;
	}
}

POLR_STRCMP_HD void polr_str_copy(uint8_t *dst_, const uint8_t *src_, uint32_t len, uint32_t lane, uint32_t n_lanes) {
	const uint64_t dst = (uint64_t)dst_, src = (uint64_t)src_;
	if (len < 8u) { // (never a heap string; byte by byte, from the words that hold the string)
		if (lane == 0u) {
			uint64_t at = 1, word = 0;
			for (uint32_t i = 0; i < len; i++) {
				const uint64_t a = (src + i) & ~7ull;
				if (a != at) {
					at = a;
					word = *(const POLR_STRCMP_MEM uint64_t *)a;
				}
				*(POLR_STRCMP_MEM uint8_t *)(dst + i) = (uint8_t)(word >> (8u * (uint32_t)((src + i) & 7ull)));
			}
		}
		return;
	}
	const uint32_t head = (uint32_t)((0ull - dst) & 7ull); // (< 8 <= len)
	const uint32_t n_words = (len - head) >> 3;
	const uint32_t tail = head + (n_words << 3), n_tail = len - tail;
	const bool has_head = lane == 0u && head != 0u, has_tail = lane == (n_lanes > 1u ? 1u : 0u) && n_tail != 0u;
	// every load of a step before its stores: a load issued behind a store would wait for that store as well
	const uint64_t first8 = has_head ? polr_strcopy_load8(src) : 0ull;
	const uint64_t last8 = has_tail ? polr_strcopy_load8(src + len - 8ull) : 0ull;
	const uint64_t s0 = src + head;                    // the source of body word 0
	const uint32_t shift = 8u * (uint32_t)(s0 & 7ull); // (the same for every body word: they are 8 bytes apart)
	if (n_lanes == 1u) {
		// alone: four destination words a step, from the four or five aligned source words that hold their bytes
		for (uint32_t k = 0; k < n_words; k += 4u) {
			const uint32_t m = n_words - k < 4u ? n_words - k : 4u, need = m + (shift ? 1u : 0u);
			const uint64_t a = (s0 + 8ull * k) & ~7ull;
			uint64_t w[5];
#if defined(__HIPCC__)
#pragma unroll
#endif
			for (uint32_t j = 0; j < 5u; j++) {
				w[j] = j < need ? *(const POLR_STRCMP_MEM uint64_t *)(a + 8ull * j) : 0ull;
			}
			if (k == 0u) { // (the edges with the first step: their loads are done)
				if (has_head) {
					polr_strcopy_store_head(dst, first8, head);
				}
				if (has_tail) {
					polr_strcopy_store_tail(dst + tail, last8 >> (8u * (8u - n_tail)), n_tail);
				}
			}
#if defined(__HIPCC__)
#pragma unroll
#endif
			for (uint32_t j = 0; j < 4u; j++) {
				if (j < m) {
					const uint64_t v = shift ? (w[j] >> shift) | (w[j + 1u] << (64u - shift)) : w[j];
					*(POLR_STRCMP_MEM uint64_t *)(dst + head + 8ull * (k + j)) = v;
				}
			}
		}
		if (n_words != 0u) {
			return;
		}
	}
	if (has_head) {
		polr_strcopy_store_head(dst, first8, head);
	}
	if (has_tail) {
		polr_strcopy_store_tail(dst + tail, last8 >> (8u * (8u - n_tail)), n_tail);
	}
	if (n_lanes > 1u) {
		for (uint32_t k = lane; k < n_words; k += n_lanes) {
			*(POLR_STRCMP_MEM uint64_t *)(dst + head + 8ull * k) = polr_strcopy_load8(s0 + 8ull * k);
		}
	}
}
