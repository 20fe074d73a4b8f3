// tests/devbuf/devbuf_main.cpp -- the contract of DevBuf (duckdb-polr_amd/csrc/polr_devbuf.h) on a host, without a GPU:
// hipMalloc / hipFree are defined here over malloc / free, keep the set of live blocks, count their calls and can make
// the n-th allocation fail.  Every step ends with check(): the live-byte count of the header equals the sum of the live
// blocks.  Prints the counts and "ok" (tests/test_devbuf.py asserts them); any violation aborts with a message.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <utility>
#include <vector>

#include "../../duckdb-polr_amd/csrc/polr_devbuf.h"

static std::map<void *, size_t> g_live;
static uint64_t g_mallocs = 0, g_frees = 0, g_failed = 0, g_null_frees = 0, g_bad_frees = 0, g_steps = 0;
static uint64_t g_fail_at = 0; // the g_fail_at-th hipMalloc call from now fails (0: none)

hipError_t hipMalloc(void **ptr, size_t bytes) {
	if (g_fail_at && --g_fail_at == 0) {
		g_failed++;
		*ptr = nullptr;
		return hipErrorOutOfMemory;
	}
	g_mallocs++;
	*ptr = malloc(bytes);
	g_live[*ptr] = bytes;
	return hipSuccess;
}

hipError_t hipFree(void *ptr) {
	if (!ptr) {
		g_null_frees++;
		return hipSuccess;
	}
	auto it = g_live.find(ptr);
	if (it == g_live.end()) {
		g_bad_frees++; // (freed twice, or never allocated)
		return hipSuccess;
	}
	g_frees++;
	g_live.erase(it);
	free(ptr);
	return hipSuccess;
}

#define REQUIRE(cond_)                                                                                                 \
	do {                                                                                                               \
		if (!(cond_)) {                                                                                                \
			fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond_);                                   \
			exit(1);                                                                                                   \
		}                                                                                                              \
	} while (0)

static uint64_t live_sum() {
	uint64_t s = 0;
	for (auto &b : g_live) {
		s += b.second;
	}
	return s;
}

// after every step: the header's count is the sum of the live blocks; nothing was freed twice or as a null pointer
#define CHECK()                                                                                                        \
	do {                                                                                                               \
		g_steps++;                                                                                                     \
		REQUIRE(polr_devbuf_live_bytes.load() == live_sum());                                                          \
		REQUIRE(g_null_frees == 0 && g_bad_frees == 0);                                                                \
	} while (0)

int main() {
	CHECK();
	{ // alloc, sizes, reset; an empty buffer frees nothing
		DevBuf<uint32_t> a;
		REQUIRE(a.get() == nullptr && a.size() == 0 && a.bytes() == 0);
		a.reset();
		CHECK();
		REQUIRE(a.alloc(10) == hipSuccess);
		REQUIRE(a.get() && a.size() == 10 && a.bytes() == 40 && g_live.at(a.get()) == 40);
		uint32_t *view = a; // (a buffer converts to its pointer)
		REQUIRE(view == a.get());
		CHECK();
		void *old = a.get();
		REQUIRE(a.alloc(3) == hipSuccess); // frees what it holds first
		REQUIRE(!g_live.count(old) || a.get() == old);
		REQUIRE(g_live.size() == 1 && a.bytes() == 12);
		CHECK();
		a.reset();
		REQUIRE(a.get() == nullptr && a.size() == 0 && a.bytes() == 0 && g_live.empty());
		CHECK();
		a.reset(); // twice: no call
		CHECK();
	}
	REQUIRE(g_mallocs == 2 && g_frees == 2);
	{ // a request for zero bytes allocates 16
		DevBuf<uint64_t> z;
		REQUIRE(z.alloc(0) == hipSuccess);
		REQUIRE(z.get() && z.size() == 0 && z.bytes() == 16 && g_live.at(z.get()) == 16);
		CHECK();
		REQUIRE(z.ensure(0) == hipSuccess && g_mallocs == 3); // (already there)
		CHECK();
	}
	REQUIRE(g_live.empty() && g_frees == 3);
	CHECK();
	{ // a failed alloc / ensure leaves an empty buffer and has freed the old block
		DevBuf<uint8_t> f;
		REQUIRE(f.alloc(100) == hipSuccess);
		g_fail_at = 1;
		REQUIRE(f.alloc(200) == hipErrorOutOfMemory);
		REQUIRE(f.get() == nullptr && f.size() == 0 && f.bytes() == 0 && g_live.empty());
		CHECK();
		REQUIRE(f.ensure(50) == hipSuccess && f.size() == 50); // the next call grows it again
		g_fail_at = 1;
		REQUIRE(f.ensure(51) == hipErrorOutOfMemory);
		REQUIRE(f.get() == nullptr && f.size() == 0 && f.bytes() == 0 && g_live.empty());
		CHECK();
		g_fail_at = 1;
		REQUIRE(f.ensure(0) == hipErrorOutOfMemory && f.get() == nullptr); // (an empty buffer holds nothing, not even 0 elements)
		CHECK();
	}
	REQUIRE(g_failed == 3 && g_mallocs == 5 && g_frees == 5);
	{ // ensure with enough capacity makes no call and keeps the block; a larger request replaces it
		DevBuf<uint16_t> e;
		REQUIRE(e.ensure(64) == hipSuccess);
		void *p = e.get();
		const uint64_t m = g_mallocs, f = g_frees;
		REQUIRE(e.ensure(64) == hipSuccess && e.ensure(1) == hipSuccess && e.ensure(0) == hipSuccess);
		REQUIRE(e.get() == p && e.size() == 64 && g_mallocs == m && g_frees == f);
		CHECK();
		REQUIRE(e.ensure(65) == hipSuccess);
		REQUIRE(e.size() == 65 && e.bytes() == 130 && g_mallocs == m + 1 && g_frees == f + 1 && g_live.size() == 1);
		CHECK();
	}
	CHECK();
	{ // move construction and move assignment hand the block over: no call, no double free
		DevBuf<uint32_t> a;
		REQUIRE(a.alloc(7) == hipSuccess);
		void *p = a.get();
		const uint64_t m = g_mallocs, f = g_frees;
		DevBuf<uint32_t> b(std::move(a));
		REQUIRE(a.get() == nullptr && a.size() == 0 && a.bytes() == 0);
		REQUIRE(b.get() == p && b.size() == 7 && b.bytes() == 28 && g_mallocs == m && g_frees == f);
		CHECK();
		DevBuf<uint32_t> c;
		c = std::move(b); // onto an empty buffer
		REQUIRE(b.get() == nullptr && c.get() == p && g_mallocs == m && g_frees == f);
		CHECK();
		DevBuf<uint32_t> d;
		REQUIRE(d.alloc(9) == hipSuccess);
		void *q = d.get();
		d = std::move(c); // onto a full buffer: its old block goes
		REQUIRE(c.get() == nullptr && d.get() == p && d.size() == 7 && !g_live.count(q) && g_frees == f + 1);
		CHECK();
		DevBuf<uint32_t> &self = d;
		d = std::move(self); // onto itself: nothing
		REQUIRE(d.get() == p && d.size() == 7 && g_frees == f + 1);
		CHECK();
	}
	REQUIRE(g_live.empty());
	CHECK();
	{ // release hands the pointer out: the destructor frees nothing, the count no longer holds it
		void *p = nullptr;
		const uint64_t f = g_frees;
		{
			DevBuf<uint8_t> r;
			REQUIRE(r.alloc(33) == hipSuccess);
			p = r.release();
			REQUIRE(p && r.get() == nullptr && r.size() == 0 && r.bytes() == 0);
			REQUIRE(polr_devbuf_live_bytes.load() == 0);
		}
		REQUIRE(g_frees == f && g_live.count(p) == 1);
		REQUIRE(hipFree(p) == hipSuccess); // (the caller's now)
		DevBuf<uint8_t> none;
		REQUIRE(none.release() == nullptr);
		CHECK();
	}
	{ // a vector of buffers that reallocates frees nothing early; its destruction frees every block once
		const uint64_t m = g_mallocs, f = g_frees;
		{
			std::vector<DevBuf<uint8_t>> v;
			std::vector<void *> ptrs;
			for (int i = 0; i < 100; i++) {
				DevBuf<uint8_t> b;
				REQUIRE(b.alloc(1 + i) == hipSuccess);
				ptrs.push_back(b.get());
				v.push_back(std::move(b));
				REQUIRE(g_frees == f && g_live.size() == (size_t)i + 1);
			}
			for (int i = 0; i < 100; i++) {
				REQUIRE(v[i].get() == ptrs[i] && v[i].size() == (uint64_t)1 + i);
			}
			CHECK();
			v.resize(150); // (empty buffers behind the full ones)
			v.erase(v.begin()); // every element moves down by one: one block goes
			REQUIRE(g_frees == f + 1 && v[0].get() == ptrs[1]);
			CHECK();
		}
		REQUIRE(g_mallocs == m + 100 && g_frees == f + 100 && g_live.empty());
		CHECK();
	}
	REQUIRE(polr_devbuf_live_bytes.load() == 0 && g_live.empty());
	REQUIRE(g_mallocs == g_frees); // (the released block included: freed by hand above)
	printf("%llu allocations, %llu frees, %llu failed allocations, %llu null frees, %llu bad frees, %llu live blocks, "
	       "%llu live bytes, %llu steps checked\n",
	       (unsigned long long)g_mallocs, (unsigned long long)g_frees, (unsigned long long)g_failed,
	       (unsigned long long)g_null_frees, (unsigned long long)g_bad_frees, (unsigned long long)g_live.size(),
	       (unsigned long long)polr_devbuf_live_bytes.load(), (unsigned long long)g_steps);
	printf("ok\n");
	return 0;
}
