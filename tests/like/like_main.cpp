// tests/like/like_main.cpp -- the LIKE matcher of duckdb-polr_amd/csrc/polr_like.h over patterns lowered by
// duckdb-polr_amd/csrc/polr_filter_plan.h, as a stand-alone host program.
//
//   like_match <file>    file: u32 n, n x (u32 length, bytes) patterns; u32 m, m x (u32 length, bytes) strings
//                        (tests/test_like_match.py writes tests/scanexpr.py's LIKE_EDGES)
//   prints one line per pattern: one character '0' / '1' per string
//
// Every string is matched in every form a cell can take: inline (length <= 12) with zero padding and with garbage
// padding; long at every alignment 0..7 of its heap copy.  A heap copy lives in an allocation of exactly the aligned
// 8-byte words that contain the string -- what the matcher may read --, the bytes around the string filled with garbage;
// the lowered pattern's segments and bytes live in allocations of exactly their size.  All forms must agree.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../duckdb-polr_amd/csrc/polr_filter_plan.h"
#include "../../duckdb-polr_amd/csrc/polr_like.h"

static bool read_list(FILE *f, std::vector<std::string> &out) {
	uint32_t n = 0;
	if (fread(&n, 4, 1, f) != 1) {
		return false;
	}
	for (uint32_t i = 0; i < n; i++) {
		uint32_t len = 0;
		if (fread(&len, 4, 1, f) != 1) {
			return false;
		}
		std::string s(len, '\0');
		if (len && fread(&s[0], 1, len, f) != len) {
			return false;
		}
		out.push_back(s);
	}
	return true;
}

template <class T>
static T *exact_copy(const T *src, size_t n) {
	T *p = (T *)malloc(n ? n * sizeof(T) : 1);
	if (n) {
		memcpy(p, src, n * sizeof(T));
	}
	return p;
}

int main(int argc, char **argv) {
	if (argc != 2) {
		fprintf(stderr, "usage: %s <patterns and strings file>\n", argv[0]);
		return 2;
	}
	FILE *f = fopen(argv[1], "rb");
	if (!f) {
		perror(argv[1]);
		return 2;
	}
	std::vector<std::string> patterns, strs;
	if (!read_list(f, patterns) || !read_list(f, strs)) {
		return 2;
	}
	fclose(f);
	const PolrFilterColumn col = {16, 0};
	unsigned long long forms = 0, disagreements = 0;
	for (const std::string &pat : patterns) {
		polr_filter_node node = {POLR_FX_LIKE, 0, 0, 0, 1, 0};
		polr_filter_value value = {0, pat.data(), pat.size()};
		PolrFilterPlan pl;
		const int rc = polr_filter_plan(&node, 1, &value, 1, &col, 1, pl);
		if (rc != POLR_OK) {
			fprintf(stderr, "pattern refused (%d): %s\n", rc, pl.err);
			return 2;
		}
		polr_like_seg *segs = exact_copy(pl.segs.data(), pl.segs.size());
		uint8_t *bytes = exact_copy(pl.bytes.data(), pl.bytes.size());
		const polr_like_pat lp = pl.values[0].pat;
		std::string line;
		for (const std::string &s : strs) {
			const uint32_t len = (uint32_t)s.size();
			int verdict = -1;
			const int n_forms = len < 12 ? 2 : (len == 12 ? 1 : 8);
			for (int form = 0; form < n_forms; form++) {
				uint8_t raw[16];
				uint8_t *heap = nullptr;
				memset(raw, form ? 0xA5 : 0x00, sizeof(raw));
				memcpy(raw, &len, 4);
				if (len <= 12) {
					memcpy(raw + 4, s.data(), len);
				} else {
					const size_t region = ((size_t)form + len + 7) & ~(size_t)7;
					heap = (uint8_t *)aligned_alloc(8, region);
					memset(heap, 0x5A, region);
					memcpy(heap + form, s.data(), len);
					memcpy(raw + 4, s.data(), 4);
					const uint64_t ptr = (uint64_t)(uintptr_t)(heap + form);
					memcpy(raw + 8, &ptr, 8);
				}
				uint32_t w[4];
				memcpy(w, raw, 16);
				const int got = polr_like_match(w[0], w[1], w[2], w[3], lp, segs, bytes) ? 1 : 0;
				free(heap);
				forms++;
				if (verdict >= 0 && got != verdict) {
					disagreements++;
					fprintf(stderr, "forms disagree: pattern of %zu bytes, string of %u bytes, form %d\n", pat.size(), len, form);
				}
				verdict = got;
			}
			line += verdict ? '1' : '0';
		}
		free(segs);
		free(bytes);
		printf("%s\n", line.c_str());
	}
	printf("%zu patterns, %zu strings, %llu forms matched, %llu disagreements\n", patterns.size(), strs.size(), forms,
	       disagreements);
	if (disagreements) {
		return 1;
	}
	printf("ok\n");
	return 0;
}
