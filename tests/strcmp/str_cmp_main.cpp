// tests/strcmp/str_cmp_main.cpp -- the string_t-against-constant comparison of duckdb-polr_amd/csrc/polr_strcmp.h as a
// stand-alone host program: every ordered pair (cell, constant) of a set of strings against memcmp-then-length
// (the reference's StringComparisonOperators, comparison_operators.hpp:157-227).
//
//   str_cmp <file>     file: u32 n, then n x (u32 length, bytes) -- tests/test_str_compare.py writes tests/scanstr.py's EDGES
//
// Every string lives in an allocation of exactly its size (the heap copy of a long cell, the bytes a constant is made
// from, the constant's tail beyond 12 bytes), so the address sanitizer sees any byte read past an end.  Inline cells are
// compared twice: padding zero, and padding filled with non-zero garbage.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../duckdb-polr_amd/csrc/polr_strcmp.h"

struct Exact { // a copy in an allocation of exactly n bytes
	uint8_t *p;
	explicit Exact(const std::string &s, size_t from = 0) : p(nullptr) {
		if (s.size() > from) {
			p = (uint8_t *)malloc(s.size() - from);
			memcpy(p, s.data() + from, s.size() - from);
		}
	}
	~Exact() {
		free(p);
	}
	Exact(const Exact &) = delete;
};

struct Cell {
	uint32_t w[4];
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
	unsigned long long pairs = 0, bad = 0, inline_cells = 0, heap_cells = 0;
	for (const std::string &a : strs) {
		const Exact heap(a);
		for (int variant = 0; variant < 2; variant++) {
			if (variant == 1 && a.size() >= 12) {
				continue; // (no padding to fill)
			}
			const Cell cell = make_cell(a, heap.p, variant ? 0xA5 : 0x00);
			(a.size() <= 12 ? inline_cells : heap_cells)++;
			for (const std::string &b : strs) {
				const Exact src(b), tail(b, 12);
				const polr_str_const c = polr_str_const_make(src.p, b.size());
				const int got = polr_str_cmp3(cell.w[0], cell.w[1], cell.w[2], cell.w[3], c, tail.p);
				const int want = reference(a, b);
				const int sign = got < 0 ? -1 : (got > 0 ? 1 : 0);
				const bool holds[6] = {want == 0, want != 0, want < 0, want > 0, want <= 0, want >= 0};
				bool ok = sign == want;
				for (uint32_t op = 0; op < 6; op++) {
					ok = ok && polr_str_cmp_holds(got, op) == holds[op];
				}
				pairs++;
				if (!ok) {
					bad++;
					if (bad <= 10) {
						printf("MISMATCH cell len %zu (padding %d) vs constant len %zu: got %d, want %d\n", a.size(), variant, b.size(),
						       got, want);
					}
				}
			}
		}
	}
	printf("%u strings, %llu inline cells, %llu heap cells, %llu pairs compared, %llu mismatches\n", n, inline_cells, heap_cells,
	       pairs, bad);
	if (bad) {
		return 1;
	}
	printf("ok\n");
	return 0;
}
