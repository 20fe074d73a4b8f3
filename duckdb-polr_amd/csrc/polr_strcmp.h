// duckdb-polr_amd/csrc/polr_strcmp.h -- the order of a string_t cell against a constant, and of two cells (polr_str_cell_cmp3,
// below), defined once for host and device.
//
// Reference: StringComparisonOperators / templated_string_compare_op (src/include/duckdb/common/operator/
// comparison_operators.hpp:157-227): memcmp over the shorter of the two lengths, bytes unsigned; on a tie the shorter
// string is the smaller one (:203-208); equality is "same length, same bytes".  '\0' and 0x80-0xFF are ordinary bytes, no
// collation.  str_less of polr_strheap.hip (the string MIN / MAX sink) is the byte-loop form of the same order between two
// cells: both implement comparison_operators.hpp:203-208.
//
// A cell (string_type.hpp:23-28) is four little-endian words: the length, then either up to 12 characters (length <= 12;
// the bytes behind the string are padding and may hold anything) or the first four characters and an 8-byte pointer to
// all of them.  The constant is prepared once on the host (polr_str_const_make): its length and its first 12 bytes as
// three words padded with zeros; what lies beyond 12 bytes stays in memory (`tail`).
//
// Why words suffice.  Let n = min(cell length, constant length).  Mask every word of the cell to the bytes that belong
// to its string (the constant's words are zero-padded already) and swap both to big-endian, so that the order of two
// words as integers is the order of their four bytes as a string.  Walk the words from the front:
//   * the first pair that differs, differs first at some byte position j.  j < n: both bytes are characters, and it is
//     the byte memcmp would have stopped at -- same verdict.  j >= n: every byte before n is equal (memcmp ties), and
//     one side has ended there (its masked byte is 0) while the other holds a non-zero character at j >= n, so that
//     side is the longer one: the word order says "the ended one is smaller", which is the length tie-break.
//   * no pair differs: all n shared bytes are equal, memcmp ties, the lengths decide.  (The masked words of "ab" and
//     "ab\0" are the same words: only the lengths tell them apart, hence the tie-break is not optional.  A string that
//     is a prefix of the other, and embedded NULs, are these two cases.)
// An inline cell has all its characters in words 0-2; against a constant longer than 12 bytes a tie over the three
// words means the cell is a prefix of the constant, and the lengths decide without the tail.  A long cell has only word
// 0 (four characters, never masked); if that ties and the constant has more than four bytes, the characters from 4 on
// are read through the pointer -- the only case that touches the heap.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define POLR_STRCMP_HD __host__ __device__ __forceinline__
#else
#define POLR_STRCMP_HD static inline
#endif
// (device code names the address space of the heap and the tail: GLOBAL_ loads, not FLAT_ ones -- polr_device.h)
#if defined(__HIP_DEVICE_COMPILE__)
#define POLR_STRCMP_MEM __attribute__((address_space(1)))
#else
#define POLR_STRCMP_MEM
#endif

struct polr_str_const {
	uint32_t len;
	uint32_t w[3]; // bytes 0-11 as the cell would hold them (little-endian), zero beyond len
};

POLR_STRCMP_HD polr_str_const polr_str_const_make(const uint8_t *s, uint64_t len) {
	polr_str_const c;
	c.len = (uint32_t)len;
	c.w[0] = c.w[1] = c.w[2] = 0;
	for (uint32_t i = 0; i < 12u && i < len; i++) {
		c.w[i >> 2] |= (uint32_t)s[i] << (8u * (i & 3u));
	}
	return c;
}

// the bytes of word `i` (0-2) that belong to a string of `len` bytes
POLR_STRCMP_HD uint32_t polr_str_word_mask(uint32_t len, uint32_t i) {
	const uint32_t left = len > 4u * i ? len - 4u * i : 0u;
	return left >= 4u ? 0xFFFFFFFFu : (left ? (1u << (8u * left)) - 1u : 0u);
}

POLR_STRCMP_HD uint32_t polr_str_bswap(uint32_t v) {
	return __builtin_bswap32(v);
}

// < 0, 0, > 0: the cell's string is smaller than, equal to, greater than the constant.  the cell = len, w0, w1, w2;
// tail = the constant's bytes from 12 on (read only when c.len > 12; may be NULL otherwise).
POLR_STRCMP_HD int polr_str_cmp3(uint32_t len, uint32_t w0, uint32_t w1, uint32_t w2, const polr_str_const &c,
                                 const uint8_t *tail) {
	const int by_length = len < c.len ? -1 : (len > c.len ? 1 : 0);
	if (len <= 12u) {
		const uint32_t a0 = polr_str_bswap(w0 & polr_str_word_mask(len, 0)), b0 = polr_str_bswap(c.w[0]);
		if (a0 != b0) {
			return a0 < b0 ? -1 : 1;
		}
		const uint32_t a1 = polr_str_bswap(w1 & polr_str_word_mask(len, 1)), b1 = polr_str_bswap(c.w[1]);
		if (a1 != b1) {
			return a1 < b1 ? -1 : 1;
		}
		const uint32_t a2 = polr_str_bswap(w2 & polr_str_word_mask(len, 2)), b2 = polr_str_bswap(c.w[2]);
		if (a2 != b2) {
			return a2 < b2 ? -1 : 1;
		}
		return by_length;
	}
	// long cell: the prefix is four characters
	const uint32_t a0 = polr_str_bswap(w0), b0 = polr_str_bswap(c.w[0]);
	if (a0 != b0) {
		return a0 < b0 ? -1 : 1;
	}
	if (c.len <= 4u) {
		return 1; // the constant is a prefix of the cell's string (len > 12 >= c.len)
	}
	const POLR_STRCMP_MEM uint8_t *s = (const POLR_STRCMP_MEM uint8_t *)(((uint64_t)w2 << 32) | w1);
	const POLR_STRCMP_MEM uint8_t *t = (const POLR_STRCMP_MEM uint8_t *)tail;
	const uint32_t n = len < c.len ? len : c.len;
	for (uint32_t i = 4; i < n; i++) {
		const uint32_t x = s[i];
		const uint32_t y = i < 12u ? (c.w[i >> 2] >> (8u * (i & 3u))) & 0xFFu : (uint32_t)t[i - 12u];
		if (x != y) {
			return x < y ? -1 : 1;
		}
	}
	return by_length;
}

// byte i (4 <= i < len) of a cell's string: an inline cell holds it in w1 / w2, a long one behind its pointer
POLR_STRCMP_HD uint32_t polr_str_cell_byte(uint32_t len, uint32_t w1, uint32_t w2, uint32_t i) {
	if (len <= 12u) {
		return ((i < 8u ? w1 : w2) >> (8u * (i & 3u))) & 0xFFu;
	}
	const POLR_STRCMP_MEM uint8_t *s = (const POLR_STRCMP_MEM uint8_t *)(((uint64_t)w2 << 32) | w1);
	return s[i];
}

// < 0, 0, > 0: the string of cell a is smaller than, equal to, greater than the string of cell b -- the same order between
// two cells (the order of the sorted dictionary codes, polr_dict.hip).  A cell = len, w0, w1, w2 as above.  Two inline
// cells are three masked big-endian words and the lengths, by the argument at the top.  Otherwise word 0 decides where it
// differs (an inline cell's masked to its own bytes, a long cell's four characters); where it ties, the bytes from 4 up to
// the shorter length are compared one by one -- from the words of an inline cell, through the pointer of a long one, never
// past either string -- and then the lengths.
POLR_STRCMP_HD int polr_str_cell_cmp3(uint32_t alen, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t blen, uint32_t b0,
                                      uint32_t b1, uint32_t b2) {
	const int by_length = alen < blen ? -1 : (alen > blen ? 1 : 0);
	const uint32_t x0 = polr_str_bswap(a0 & polr_str_word_mask(alen, 0)), y0 = polr_str_bswap(b0 & polr_str_word_mask(blen, 0));
	if (x0 != y0) {
		return x0 < y0 ? -1 : 1;
	}
	if (alen <= 12u && blen <= 12u) {
		const uint32_t x1 = polr_str_bswap(a1 & polr_str_word_mask(alen, 1)), y1 = polr_str_bswap(b1 & polr_str_word_mask(blen, 1));
		if (x1 != y1) {
			return x1 < y1 ? -1 : 1;
		}
		const uint32_t x2 = polr_str_bswap(a2 & polr_str_word_mask(alen, 2)), y2 = polr_str_bswap(b2 & polr_str_word_mask(blen, 2));
		if (x2 != y2) {
			return x2 < y2 ? -1 : 1;
		}
		return by_length;
	}
	const uint32_t n = alen < blen ? alen : blen;
	for (uint32_t i = 4; i < n; i++) {
		const uint32_t x = polr_str_cell_byte(alen, a1, a2, i), y = polr_str_cell_byte(blen, b1, b2, i);
		if (x != y) {
			return x < y ? -1 : 1;
		}
	}
	return by_length;
}

#if defined(__HIPCC__)
// byte i (i < length) of the string of a cell held as a uint4: what str_less compares and the string records are written
// from (polr_str_records_kernel; both polr_strheap.hip)
__device__ __forceinline__ uint32_t str_byte(const uint4 &c, uint32_t i) {
	if (c.x <= 12u) {
		const uint32_t w = i < 4 ? c.y : (i < 8 ? c.z : c.w);
		return (w >> (8u * (i & 3u))) & 0xFFu;
	}
	if (i < 4) {
		return (c.y >> (8u * i)) & 0xFFu;
	}
	const uint8_t *p = (const uint8_t *)(((uint64_t)c.w << 32) | c.z);
	return p[i];
}
#endif

// does a three-way result satisfy a comparison code of include/polr_hip.h (POLR_CMP_EQ = 0 .. POLR_CMP_GE = 5)?
POLR_STRCMP_HD bool polr_str_cmp_holds(int r, uint32_t op) {
	return op == 0u ? r == 0 : op == 1u ? r != 0 : op == 2u ? r < 0 : op == 3u ? r > 0 : op == 4u ? r <= 0 : r >= 0;
}
