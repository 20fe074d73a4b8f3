// tests/devbuf/hip/hip_runtime.h -- a stand-in for the HIP runtime header, just large enough to compile
// duckdb-polr_amd/csrc/polr_devbuf.h on a host: devbuf_main.cpp defines the two functions over malloc / free.
#pragma once

#include <stddef.h>

typedef enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 } hipError_t;

hipError_t hipMalloc(void **ptr, size_t bytes);
hipError_t hipFree(void *ptr);
