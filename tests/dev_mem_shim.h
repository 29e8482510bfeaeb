// The five runtime calls pauxy_amd/csrc/dev_guard.h and dev_mem.h are written over, on the host (AFQ_DEV_MEM_HOST_SHIM):
// "device" memory is host memory, allocated to the byte and page-aligned as hipMalloc's is, so that a sanitizer sees every
// access of the guard logic outside what it asked for.  shim_last_* let a test see what was asked for.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };

inline size_t shim_last_bytes = 0, shim_mallocs = 0, shim_frees = 0, shim_syncs = 0;
inline void *shim_last_ptr = nullptr;

inline hipError_t hipMalloc(void **p, size_t bytes) {
    *p = nullptr;
    if (posix_memalign(p, 4096, bytes ? bytes : 1)) return hipErrorOutOfMemory;
    shim_last_bytes = bytes; shim_last_ptr = *p; ++shim_mallocs;
    return hipSuccess;
}
inline hipError_t hipFree(void *p) { free(p); ++shim_frees; return hipSuccess; }
inline hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind) { memcpy(dst, src, n); return hipSuccess; }
inline hipError_t hipMemsetD32(void *dst, uint32_t word, size_t count) {
    uint32_t *d = (uint32_t *)dst;
    for (size_t i = 0; i < count; ++i) d[i] = word;
    return hipSuccess;
}
inline hipError_t hipDeviceSynchronize() { ++shim_syncs; return hipSuccess; }
