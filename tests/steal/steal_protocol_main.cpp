// tests/steal/steal_protocol_main.cpp -- the claim / steal protocol of duckdb-polr_amd/csrc/polr_steal.h on the host:
// known answers on one thread, then 8 threads as executors over 4 096 chunks.  tests/test_steal_protocol.py builds
// this with the thread sanitizer and with the address + undefined-behaviour sanitizers and runs the binaries.
// Exit status 0 and a last line "ok": every check held.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <thread>
#include <utility>
#include <vector>

#include "../../duckdb-polr_amd/csrc/polr_steal.h"

using namespace polr_steal;

static int g_failed = 0;
#define CHECK(cond_)                                                                                                   \
	do {                                                                                                               \
		if (!(cond_)) {                                                                                                \
			fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond_);                                  \
			g_failed++;                                                                                                \
		}                                                                                                              \
	} while (0)

static void known_answers() {
	uint32_t b = 0, e = 0;
	{ // {0, 10}, grant 3: [0,3) [3,6) [6,9) [9,10), then nothing
		Word w(pack(0, 10));
		const uint32_t want[4][2] = {{0, 3}, {3, 6}, {6, 9}, {9, 10}};
		for (int i = 0; i < 4; i++) {
			CHECK(claim(&w, 3, &b, &e));
			CHECK(b == want[i][0] && e == want[i][1]);
		}
		CHECK(!claim(&w, 3, &b, &e));
		CHECK(!claim(&w, 3, &b, &e));
		CHECK(word_load(&w) == pack(10, 10));
	}
	{ // a steal from {2, 10} at grant 2 leaves the victim {2, 6} and returns [6, 10), which the thief's word then holds
		Word w[2];
		word_store(&w[0], pack(2, 10));
		word_store(&w[1], pack(40, 40));
		CHECK(steal(w, 2, 1, 2, &b, &e));
		CHECK(b == 6 && e == 10);
		CHECK(word_load(&w[0]) == pack(2, 6));
		CHECK(word_load(&w[1]) == pack(6, 10));
		CHECK(claim(&w[1], 2, &b, &e) && b == 6 && e == 8);
	}
	{ // {7, 10} at grant 2: three chunks left, half of them is less than a grant -- refused, nothing changes
		Word w[2];
		word_store(&w[0], pack(7, 10));
		word_store(&w[1], pack(0, 0));
		CHECK(!steal(w, 2, 1, 2, &b, &e));
		CHECK(word_load(&w[0]) == pack(7, 10));
		CHECK(word_load(&w[1]) == pack(0, 0));
		CHECK(steal_amount(3, 2) == 0 && steal_amount(4, 2) == 2 && steal_amount(7, 2) == 2 && steal_amount(8, 2) == 4);
		CHECK(steal_amount(1, 1) == 0 && steal_amount(2, 1) == 1 && steal_amount(4095, 64) == 1984);
	}
	{ // victim choice: the largest remainder, the lowest index on ties, never the thief itself
		Word w[6];
		const uint64_t init[6] = {pack(0, 8), pack(100, 120), pack(200, 220), pack(300, 310), pack(400, 400), pack(500, 520)};
		for (int i = 0; i < 6; i++) {
			word_store(&w[i], init[i]);
		}
		uint32_t victim = 99;
		uint64_t seen = 0;
		CHECK(pick_victim(w, 6, 4, &victim, &seen) && victim == 1 && seen == pack(100, 120));
		CHECK(pick_victim(w, 6, 1, &victim, &seen) && victim == 2 && seen == pack(200, 220));
		CHECK(steal(w, 6, 4, 4, &b, &e) && b == 112 && e == 120);
		CHECK(word_load(&w[1]) == pack(100, 112) && word_load(&w[4]) == pack(112, 120));
		// now 2 and 5 tie at 20: the lower index
		CHECK(pick_victim(w, 6, 3, &victim, &seen) && victim == 2);
		// a compare-and-swap on a value that is no longer there loses and changes nothing
		CHECK(take(w, 1, pack(100, 120), 3, 4, &b, &e) == 0);
		CHECK(word_load(&w[1]) == pack(100, 112) && word_load(&w[3]) == pack(300, 310));
	}
}

struct Layout {
	const char *name;
	std::vector<std::pair<uint32_t, uint32_t>> ranges; // one per executor
};

// every thread: claim, else steal, else leave; every claimed chunk bumps its counter
static void run_layout(const Layout &lay, uint32_t grant, uint32_t n_chunks) {
	const uint32_t n = (uint32_t)lay.ranges.size();
	std::vector<Word> words(n);
	std::vector<std::atomic<uint32_t>> hits(n_chunks);
	std::vector<uint8_t> in_union(n_chunks, 0);
	uint64_t union_size = 0;
	for (uint32_t i = 0; i < n; i++) {
		word_store(&words[i], pack(lay.ranges[i].first, lay.ranges[i].second));
		for (uint32_t c = lay.ranges[i].first; c < lay.ranges[i].second; c++) {
			in_union[c] = 1;
			union_size++;
		}
	}
	for (auto &h : hits) {
		h.store(0, std::memory_order_relaxed);
	}
	std::vector<uint64_t> claimed(n, 0), stolen(n, 0);
	std::vector<uint8_t> finished(n, 0);
	std::atomic<uint32_t> go(0);
	std::vector<std::thread> threads;
	for (uint32_t t = 0; t < n; t++) {
		threads.emplace_back([&, t]() {
			go.fetch_add(1);
			while (go.load() < n) { // (start together, so that thieves and owners really meet)
				std::this_thread::yield();
			}
			uint32_t b = 0, e = 0;
			while (true) {
				if (claim(&words[t], grant, &b, &e)) {
					if (e - b > grant || e <= b) {
						fprintf(stderr, "%s: a claim of %u chunks at grant %u\n", lay.name, e - b, grant);
						abort();
					}
					for (uint32_t c = b; c < e; c++) {
						hits[c].fetch_add(1, std::memory_order_relaxed);
					}
					claimed[t] += e - b;
					continue;
				}
				if (!steal(words.data(), n, t, grant, &b, &e)) {
					break;
				}
				if ((e - b) % grant != 0 || e <= b) {
					fprintf(stderr, "%s: a steal of %u chunks at grant %u\n", lay.name, e - b, grant);
					abort();
				}
				stolen[t] += e - b;
			}
			finished[t] = 1;
		});
	}
	for (auto &th : threads) {
		th.join();
	}
	uint64_t sum_claimed = 0, sum_stolen = 0, wrong = 0;
	for (uint32_t t = 0; t < n; t++) {
		CHECK(finished[t] == 1);
		sum_claimed += claimed[t];
		sum_stolen += stolen[t];
		CHECK(remainder_of(word_load(&words[t])) == 0);
	}
	for (uint32_t c = 0; c < n_chunks; c++) {
		if (hits[c].load(std::memory_order_relaxed) != (in_union[c] ? 1u : 0u)) {
			wrong++;
		}
	}
	CHECK(wrong == 0);
	CHECK(sum_claimed == union_size);
	printf("%-10s grant %2u: %llu chunks claimed, %llu stolen, %llu miscounted\n", lay.name, grant,
	       (unsigned long long)sum_claimed, (unsigned long long)sum_stolen, (unsigned long long)wrong);
}

int main() {
	known_answers();
	const uint32_t n_chunks = 4096;
	std::vector<Layout> layouts;
	{
		Layout l{"owner0", {}};
		l.ranges.assign(8, {0u, 0u});
		l.ranges[0] = {0u, n_chunks};
		layouts.push_back(l);
	}
	{
		Layout l{"even", {}};
		for (uint32_t i = 0; i < 8; i++) {
			l.ranges.push_back({i * 512u, (i + 1) * 512u});
		}
		layouts.push_back(l);
	}
	{ // disjoint ranges with gaps, three empty owners (one of them "empty at a position")
		Layout l{"gaps", {{10, 700}, {0, 0}, {900, 901}, {1500, 3001}, {3001, 3001}, {3500, 4096}, {0, 0}, {705, 830}}};
		layouts.push_back(l);
	}
	const uint32_t grants[3] = {1, 3, 64};
	for (const Layout &l : layouts) {
		for (uint32_t g : grants) {
			run_layout(l, g, n_chunks);
		}
	}
	if (g_failed) {
		fprintf(stderr, "%d check(s) failed\n", g_failed);
		return 1;
	}
	printf("ok\n");
	return 0;
}
