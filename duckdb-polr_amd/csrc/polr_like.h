// duckdb-polr_amd/csrc/polr_like.h -- does a string_t cell match a LIKE pattern?  Defined once for host and device.
//
// Reference: TemplatedLikeOperator<'%', '_', false> (src/function/scalar/string/like.cpp:22-65), bound without ESCAPE:
// '%' matches any run of bytes (none included), '_' exactly one BYTE, every other byte itself; a backslash is an ordinary
// byte.  The reference recurses at every '%'.  Here the pattern is lowered once on the host (polr_filter_plan.h): cut at
// its '%' into segments -- runs of bytes in which '_' stands for "any byte" -- with two flags, the first segment anchored
// at the front (the pattern does not begin with '%'), the last one at the back (it does not end with '%').  Matching is
// then a walk without recursion and without a stack:
//   * a front-anchored segment matches at offset 0;
//   * every segment between takes its LEFTMOST occurrence at or behind the end of the one before (an occurrence further
//     right leaves less of the string to the segments that follow and none of them more, so leftmost loses nothing);
//   * a back-anchored segment matches at the end of the string, and must not begin before the position reached;
//   * a pattern without '%' is one segment anchored at both ends: the string's length is the segment's.
// tests/test_like_match.py compares this with a regular expression over an edge set, tests/test_scan_expr_golden.py pins
// that regular expression against the reference engine.
//
// The string's bytes.  An inline cell (length <= 12) is matched from its three character words; its padding is never
// looked at.  A long cell holds its first four characters in word 1: bytes 0-3 come from there, so a front-anchored
// segment whose first bytes differ from the cell's prefix is refused before the heap is touched (polr_strcmp.h does the
// same for comparisons).  Heap strings are unaligned: bytes from 4 on are read as the aligned 8-byte words that contain
// them, one word kept in registers, so nothing outside [pointer, pointer + length) rounded to those words is read.
#pragma once

#include <stdint.h>

#include "polr_strcmp.h"

#define POLR_LIKE_FRONT 1u // the first segment matches at offset 0
#define POLR_LIKE_BACK 2u  // the last segment matches at the end
#define POLR_LIKE_ANY 0x5Fu // '_' inside a segment: any one byte

struct polr_like_seg {
	uint32_t off, len; // bytes[off .. off + len) of the call's constant bytes
};
struct polr_like_pat {
	uint32_t first_seg, n_segs; // segs[first_seg .. first_seg + n_segs)
	uint32_t flags;             // POLR_LIKE_FRONT | POLR_LIKE_BACK
	uint32_t min_len;           // the segments' lengths together: a shorter string cannot match
};

// the cell's string as the matcher reads it
struct polr_like_str {
	uint32_t len, w1, w2, w3;
	uint64_t ptr;  // long cells: the heap address of byte 0
	uint64_t at;   // the aligned address of the word held (1: none)
	uint64_t word;
};

POLR_STRCMP_HD uint32_t polr_like_byte(polr_like_str &s, uint32_t i) {
	if (s.len <= 12u || i < 4u) {
		const uint32_t w = i < 4u ? s.w1 : (i < 8u ? s.w2 : s.w3);
		return (w >> (8u * (i & 3u))) & 0xFFu;
	}
	const uint64_t a = s.ptr + i;
	if ((a & ~7ull) != s.at) {
		s.at = a & ~7ull;
		s.word = *(const POLR_STRCMP_MEM uint64_t *)s.at;
	}
	return (uint32_t)(s.word >> (8u * (uint32_t)(a & 7ull))) & 0xFFu;
}

// the segment at offset pos of the string (the caller knows pos + seg.len <= s.len)
POLR_STRCMP_HD bool polr_like_seg_at(polr_like_str &s, uint32_t pos, const polr_like_seg seg,
                                     const POLR_STRCMP_MEM uint8_t *bytes) {
	for (uint32_t j = 0; j < seg.len; j++) {
		const uint32_t pb = bytes[seg.off + j];
		if (pb != POLR_LIKE_ANY && pb != polr_like_byte(s, pos + j)) {
			return false;
		}
	}
	return true;
}

// the cell = len, w1, w2, w3 (as polr_str_cmp3 takes it); segs / bytes: the lowered constants of the call
POLR_STRCMP_HD bool polr_like_match(uint32_t len, uint32_t w1, uint32_t w2, uint32_t w3, const polr_like_pat p,
                                    const polr_like_seg *segs_, const uint8_t *bytes_) {
	if (len < p.min_len) {
		return false;
	}
	const POLR_STRCMP_MEM polr_like_seg *segs = (const POLR_STRCMP_MEM polr_like_seg *)segs_;
	const POLR_STRCMP_MEM uint8_t *bytes = (const POLR_STRCMP_MEM uint8_t *)bytes_;
	polr_like_str s;
	s.len = len;
	s.w1 = w1;
	s.w2 = w2;
	s.w3 = w3;
	s.ptr = ((uint64_t)w3 << 32) | w2;
	s.at = 1;
	s.word = 0;
	uint32_t i = p.first_seg, last = p.first_seg + p.n_segs, pos = 0;
	const uint32_t end = last;
	if (p.flags & POLR_LIKE_FRONT) {
		const polr_like_seg seg = segs[i++];
		if (!polr_like_seg_at(s, 0, seg, bytes)) { // (seg.len <= min_len <= len)
			return false;
		}
		pos = seg.len;
	}
	if (p.flags & POLR_LIKE_BACK) {
		if (i == end) {
			return pos == len; // no '%' at all: the one segment is the whole string
		}
		last = end - 1;
	}
	for (; i < last; i++) {
		const polr_like_seg seg = segs[i];
		bool found = false;
		while (!found && pos + seg.len <= len) {
			found = polr_like_seg_at(s, pos, seg, bytes);
			pos += found ? seg.len : 1u;
		}
		if (!found) {
			return false;
		}
	}
	if (last < end) {
		const polr_like_seg seg = segs[last];
		return len - pos >= seg.len && polr_like_seg_at(s, len - seg.len, seg, bytes);
	}
	return true;
}
