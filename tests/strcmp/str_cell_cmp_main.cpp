// tests/strcmp/str_cell_cmp_main.cpp -- the string_t-against-string_t comparison of duckdb-polr_amd/csrc/polr_strcmp.h
// (polr_str_cell_cmp3, the order of the sorted dictionary codes) as a stand-alone host program: every ordered pair
// (cell, cell) of a set of strings against memcmp-then-length (the reference's StringComparisonOperators,
// comparison_operators.hpp:157-227).
//
//   str_cell_cmp <file>     file: u32 n, then n x (u32 length, bytes) -- tests/test_str_cell_order.py writes tests/scanstr.py's EDGES
//
// Every long string lives in a heap allocation of exactly its size, so the address sanitizer sees any byte read past an
// end.  A string shorter than 12 bytes makes two inline cells: padding zero, and padding filled with non-zero garbage
// (two different garbage bytes on the two sides of a pair).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../../duckdb-polr_amd/csrc/polr_strcmp.h"

struct Cell {
	uint32_t w[4];
	size_t str; // index of its string
	int padded; // inline cell with garbage padding
};

static Cell make_cell(const std::string &s, const uint8_t *heap, uint8_t padding) {
	Cell c;
	uint8_t raw[16];
	memset(raw, padding, sizeof(raw));
	const uint32_t len = (uint32_t)s.size();
	memcpy(raw, &len, 4);
	if (len <= 12) {
		memcpy(raw + 4, s.data(), len);
	} else {
		memcpy(raw + 4, s.data(), 4);
		const uint64_t ptr = (uint64_t)(uintptr_t)heap;
		memcpy(raw + 8, &ptr, 8);
	}
	memcpy(c.w, raw, 16);
	return c;
}

static int reference(const std::string &a, const std::string &b) {
	const size_t n = a.size() < b.size() ? a.size() : b.size();
	const int m = n ? memcmp(a.data(), b.data(), n) : 0;
	if (m) {
		return m < 0 ? -1 : 1;
	}
	return a.size() < b.size() ? -1 : (a.size() > b.size() ? 1 : 0);
}

int main(int argc, char **argv) {
	if (argc != 2) {
		fprintf(stderr, "usage: %s <strings file>\n", argv[0]);
		return 2;
	}
	FILE *f = fopen(argv[1], "rb");
	if (!f) {
		perror(argv[1]);
		return 2;
	}
	uint32_t n = 0;
	std::vector<std::string> strs;
	if (fread(&n, 4, 1, f) != 1) {
		return 2;
	}
	for (uint32_t i = 0; i < n; i++) {
		uint32_t len = 0;
		if (fread(&len, 4, 1, f) != 1) {
			return 2;
		}
		std::string s(len, '\0');
		if (len && fread(&s[0], 1, len, f) != len) {
			return 2;
		}
		strs.push_back(s);
	}
	fclose(f);
	// the left-hand and the right-hand cells: separate heap copies, different garbage
	std::vector<std::unique_ptr<uint8_t[]>> heaps;
	std::vector<Cell> left, right;
	unsigned long long inline_cells = 0, heap_cells = 0;
	for (int side = 0; side < 2; side++) {
		std::vector<Cell> &cells = side ? right : left;
		for (size_t i = 0; i < strs.size(); i++) {
			const std::string &s = strs[i];
			uint8_t *heap = nullptr;
			if (s.size() > 12) {
				heaps.emplace_back(new uint8_t[s.size()]);
				heap = heaps.back().get();
				memcpy(heap, s.data(), s.size());
			}
			for (int variant = 0; variant < 2; variant++) {
				if (variant == 1 && s.size() >= 12) {
					continue; // (no padding to fill)
				}
				Cell c = make_cell(s, heap, variant ? (side ? 0x5A : 0xA5) : 0x00);
				c.str = i;
				c.padded = variant;
				cells.push_back(c);
				if (side == 0) {
					(s.size() <= 12 ? inline_cells : heap_cells)++;
				}
			}
		}
	}
	unsigned long long pairs = 0, bad = 0;
	for (const Cell &a : left) {
		for (const Cell &b : right) {
			const int got = polr_str_cell_cmp3(a.w[0], a.w[1], a.w[2], a.w[3], b.w[0], b.w[1], b.w[2], b.w[3]);
			const int want = reference(strs[a.str], strs[b.str]);
			const int sign = got < 0 ? -1 : (got > 0 ? 1 : 0);
			pairs++;
			if (sign != want) {
				bad++;
				if (bad <= 10) {
					printf("MISMATCH cell len %zu (padding %d) vs cell len %zu (padding %d): got %d, want %d\n", strs[a.str].size(),
					       a.padded, strs[b.str].size(), b.padded, got, want);
				}
			}
		}
	}
	printf("%u strings, %llu inline cells, %llu heap cells, %llu pairs compared, %llu mismatches\n", n, inline_cells, heap_cells, pairs,
	       bad);
	if (bad) {
		return 1;
	}
	printf("ok\n");
	return 0;
}
