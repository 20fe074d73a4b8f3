// duckdb-polr_amd/csrc/polr_devbuf.h -- DevBuf<T>: the owner of one device allocation, and the only place of the
// library that calls hipMalloc and hipFree.  Handles hold DevBuf members and free themselves when they are deleted;
// functions keep temporaries in local DevBufs and return as soon as something fails.  Needs the HIP runtime header and
// the standard library only, so a host program can compile it alone (tests/devbuf).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

// bytes of device memory DevBufs own right now, process-wide (polr_device_bytes_live)
inline std::atomic<uint64_t> polr_devbuf_live_bytes {0};

template <class T>
class DevBuf {
public:
	DevBuf() = default;
	DevBuf(const DevBuf &) = delete;
	DevBuf &operator=(const DevBuf &) = delete;
	DevBuf(DevBuf &&o) noexcept : ptr_(o.ptr_), size_(o.size_), bytes_(o.bytes_) {
		o.forget();
	}
	DevBuf &operator=(DevBuf &&o) noexcept {
		if (this != &o) {
			reset();
			ptr_ = o.ptr_;
			size_ = o.size_;
			bytes_ = o.bytes_;
			o.forget();
		}
		return *this;
	}
	~DevBuf() {
		reset();
	}

	// Free what the buffer holds, then allocate n elements; a request for zero bytes allocates 16, so that kernels are
	// handed non-null pointers for empty tables.  After a failure the buffer is empty.
	hipError_t alloc(uint64_t n) {
		reset();
		const uint64_t bytes = n ? n * sizeof(T) : 16;
		void *p = nullptr;
		const hipError_t e = hipMalloc(&p, bytes);
		if (e != hipSuccess) {
			return e;
		}
		ptr_ = (T *)p;
		size_ = n;
		bytes_ = bytes;
		polr_devbuf_live_bytes.fetch_add(bytes, std::memory_order_relaxed);
		return hipSuccess;
	}
	// Grow on demand: nothing if the buffer already holds n elements, else alloc(n) -- the contents are NOT kept.  The
	// caller synchronises first where queued work may still read the old block.
	hipError_t ensure(uint64_t n) {
		return ptr_ && size_ >= n ? hipSuccess : alloc(n);
	}
	void reset() {
		if (ptr_) {
			hipFree(ptr_);
			polr_devbuf_live_bytes.fetch_sub(bytes_, std::memory_order_relaxed);
		}
		forget();
	}
	// hand the allocation to the caller, who frees it
	T *release() {
		T *p = ptr_;
		if (p) {
			polr_devbuf_live_bytes.fetch_sub(bytes_, std::memory_order_relaxed);
		}
		forget();
		return p;
	}

	T *get() const {
		return ptr_;
	}
	operator T *() const { // a buffer stands wherever the kernels and copies take its pointer
		return ptr_;
	}
	uint64_t size() const { // elements asked for (0 for an empty buffer, and for alloc(0))
		return size_;
	}
	uint64_t bytes() const { // bytes allocated
		return bytes_;
	}

private:
	void forget() {
		ptr_ = nullptr;
		size_ = bytes_ = 0;
	}
	T *ptr_ = nullptr;
	uint64_t size_ = 0, bytes_ = 0;
};
