// tests/strcopy/strcopy_main.cpp -- duckdb-polr_amd/csrc/polr_strcopy.h as a host program (tests/test_strcopy.py builds it
// plain and under the address + undefined-behaviour sanitizers and runs it directly).
//
//   strcopy_main <offsets file>
//
// 1. polr_str_copy: for every length of the list below x source alignment 0..7 x destination alignment 0..7 x n_lanes in
//    {1, 64} (the lanes of a wave emulated one after the other).  The source sits in an allocation of exactly the aligned
//    8-byte words that contain it, so the sanitizer sees any read the rule of the header does not allow; the destination is
//    `len` bytes between two canary-filled neighbours, so a write outside the string's own bytes shows.
// 2. polr_str_pack_offsets against the lists of the offsets file: blocks of
//      n
//      <len> <valid> <wanted offset>      (n lines)
//      <wanted total>
//    computed by the test in Python, one of them with a running total beyond 2^32.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../duckdb-polr_amd/csrc/polr_strcopy.h"

static const size_t CANARY = 64; // bytes on either side of the destination (a multiple of 8: alignments stay what they are)

static uint64_t n_copies = 0, n_bad = 0;

static void one_copy(uint32_t len, uint32_t sa, uint32_t da, uint32_t n_lanes) {
	// source: exactly the words [sa, sa + len) touches, counted from an 8-aligned base
	const size_t src_bytes = ((size_t)sa + len + 7) / 8 * 8;
	uint8_t *src_mem = (uint8_t *)aligned_alloc(8, src_bytes);
	for (size_t i = 0; i < src_bytes; i++) {
		src_mem[i] = (uint8_t)(0x80u ^ (i * 131u + len * 7u + sa)); // (the words' other bytes differ from the canaries)
	}
	const uint8_t *src = src_mem + sa;
	const size_t dst_bytes = CANARY + da + len + CANARY + 8;
	uint8_t *dst_mem = (uint8_t *)aligned_alloc(8, (dst_bytes + 7) / 8 * 8);
	memset(dst_mem, 0xC7, dst_bytes);
	uint8_t *dst = dst_mem + CANARY + da;
	for (uint32_t lane = 0; lane < n_lanes; lane++) {
		polr_str_copy(dst, src, len, lane, n_lanes);
	}
	bool ok = memcmp(dst, src, len) == 0;
	for (size_t i = 0; i < dst_bytes; i++) {
		const bool inside = i >= CANARY + da && i < CANARY + da + len;
		ok = ok && (inside || dst_mem[i] == 0xC7);
	}
	n_copies++;
	if (!ok) {
		n_bad++;
		printf("copy differs: len %u, source alignment %u, destination alignment %u, %u lanes\n", len, sa, da, n_lanes);
	}
	free(src_mem);
	free(dst_mem);
}

int main(int argc, char **argv) {
	if (argc != 2) {
		fprintf(stderr, "usage: strcopy_main <offsets file>\n");
		return 2;
	}
	std::vector<uint32_t> lens;
	for (uint32_t l = 13; l <= 80; l++) {
		lens.push_back(l);
	}
	const uint32_t cut = POLR_STRCOPY_LANE_MAX;
	for (uint32_t l : {cut - 1u, cut, cut + 1u, 4097u, 100000u}) {
		lens.push_back(l);
	}
	for (uint32_t len : lens) {
		for (uint32_t sa = 0; sa < 8; sa++) {
			for (uint32_t da = 0; da < 8; da++) {
				one_copy(len, sa, da, 1);
				one_copy(len, sa, da, 64);
			}
		}
	}
	printf("cut-over %u: %zu lengths, %" PRIu64 " copies, %" PRIu64 " differ\n", cut, lens.size(), n_copies, n_bad);

	FILE *f = fopen(argv[1], "r");
	if (!f) {
		fprintf(stderr, "cannot open %s\n", argv[1]);
		return 2;
	}
	uint64_t n_lists = 0, n_rows = 0, n_wrong = 0, n = 0, max_total = 0;
	while (fscanf(f, "%" SCNu64, &n) == 1) {
		std::vector<uint32_t> len(n);
		std::vector<uint8_t> valid(n);
		std::vector<uint64_t> want(n), got(n);
		for (uint64_t i = 0; i < n; i++) {
			unsigned v = 0;
			if (fscanf(f, "%" SCNu32 " %u %" SCNu64, &len[i], &v, &want[i]) != 3) {
				fprintf(stderr, "offsets file: list %" PRIu64 " ends early\n", n_lists);
				return 2;
			}
			valid[i] = (uint8_t)v;
		}
		uint64_t want_total = 0;
		if (fscanf(f, "%" SCNu64, &want_total) != 1) {
			fprintf(stderr, "offsets file: list %" PRIu64 " has no total\n", n_lists);
			return 2;
		}
		const uint64_t total = polr_str_pack_offsets(len.data(), valid.data(), n, got.data());
		n_wrong += total != want_total;
		for (uint64_t i = 0; i < n; i++) {
			n_wrong += got[i] != want[i];
		}
		max_total = total > max_total ? total : max_total;
		n_lists++;
		n_rows += n;
	}
	fclose(f);
	printf("%" PRIu64 " offset lists, %" PRIu64 " rows, largest total %" PRIu64 ", %" PRIu64 " wrong\n", n_lists, n_rows,
	       max_total, n_wrong);
	if (n_bad || n_wrong) {
		return 1;
	}
	printf("ok\n");
	return 0;
}
