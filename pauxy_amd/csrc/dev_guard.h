// Guard bands and typed poison for the handle's device memory (AFQ_DEBUG_GUARD, read by afq_create).
//
//   0 / unset  guard_alloc is hipMalloc of the requested bytes and guard_free is hipFree: nothing else happens.
//   1          bands: a block gets `band` bytes (a multiple of 4096, AFQ_DEBUG_GUARD_BYTES, 4096 by default) in front of the
//              requested bytes and behind them, filled with GUARD_BAND_WORD -- a NaN as a float and as either half of a
//              double.  The caller gets the inner pointer (as aligned as the band is long); the registry keeps the base that
//              hipFree needs.  The body is left as hipMalloc returned it.
//   2          bands, and the body is filled before the pointer is handed out: GUARD_BODY_WORD (a NaN again) in a block of
//              double, cplx or float, zeros in every other block.  An index or a counter is never poisoned: a poisoned index
//              would turn a harmless read of unwritten memory into a wild access.
// Both bands are compared with the pattern, after a device synchronisation, before a guarded block is freed, and by
// guard_check_owner for every live block of one owner.  What differs goes to a process-wide log: block, side, offset of the
// first differing byte relative to the block (-1 is the byte in front of it, `bytes` the first one behind it) and the word found.
//
// The logic is plain host code over five runtime calls (hipMalloc, hipFree, hipMemcpy, hipMemsetD32, hipDeviceSynchronize), so
// that it compiles against a host shim of those (AFQ_DEV_MEM_HOST_SHIM, tests/dev_mem_shim.h) and runs under a sanitizer
// without a device.
#pragma once
#ifdef AFQ_DEV_MEM_HOST_SHIM
#include "dev_mem_shim.h"
#else
#include <hip/hip_runtime.h>
#endif
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

constexpr uint32_t GUARD_BAND_WORD = 0x7ff8beefu;
constexpr uint32_t GUARD_BODY_WORD = 0x7ff8feedu;

// element types whose blocks mode 2 poisons (afq_internal.h adds cplx)
template <class T> struct DevFloating : std::is_floating_point<T> {};

struct GuardCfg {
    int mode = 0;
    size_t band = 4096;
};

inline GuardCfg guard_cfg_from_env() {
    GuardCfg c;
    const char *m = getenv("AFQ_DEBUG_GUARD");
    c.mode = m ? atoi(m) : 0;
    if (c.mode < 0 || c.mode > 2) c.mode = 0;
    const char *b = getenv("AFQ_DEBUG_GUARD_BYTES");
    const long long want = b ? atoll(b) : 0;
    if (want > 4096) c.band = ((size_t)want + 4095) / 4096 * 4096;
    return c;
}

struct GuardBlock {
    char *base;             // what hipMalloc returned
    size_t bytes, band;     // requested bytes; the back band starts at inner + bytes and ends band bytes behind its next word
    std::string name;
    const void *owner;
};

struct GuardState {
    std::mutex mu;
    std::unordered_map<void *, GuardBlock> live;     // by inner pointer
    std::atomic<long> nlive{0};
    std::vector<std::string> log;
};
inline GuardState &guard_state() { static GuardState s; return s; }

inline size_t guard_round4(size_t n) { return (n + 3) / 4 * 4; }

// byte i of a band that starts at a 4-aligned address + phase
inline unsigned char guard_band_byte(size_t i) { return (unsigned char)(GUARD_BAND_WORD >> (8 * (i & 3))); }

inline hipError_t guard_alloc(const GuardCfg &cfg, void **p, size_t bytes, bool floating, const char *name, const void *owner) {
    if (cfg.mode == 0) return hipMalloc(p, bytes);
    const size_t r4 = guard_round4(bytes);
    char *base = nullptr;
    hipError_t e = hipMalloc((void **)&base, cfg.band + r4 + cfg.band);
    if (e != hipSuccess) { *p = nullptr; return e; }
    char *inner = base + cfg.band;
    if (cfg.mode == 2 && r4) e = hipMemsetD32(inner, floating ? GUARD_BODY_WORD : 0u, r4 / 4);
    if (e == hipSuccess) e = hipMemsetD32(base, GUARD_BAND_WORD, cfg.band / 4);
    if (e == hipSuccess && r4 != bytes) {       // the back band starts inside a word
        unsigned char head[4];
        for (size_t i = bytes; i < r4; ++i) head[i - bytes] = guard_band_byte(i);
        e = hipMemcpy(inner + bytes, head, r4 - bytes, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMemsetD32(inner + r4, GUARD_BAND_WORD, cfg.band / 4);
    if (e != hipSuccess) { hipFree(base); *p = nullptr; return e; }
    GuardState &g = guard_state();
    std::lock_guard<std::mutex> lock(g.mu);
    g.live[inner] = GuardBlock{base, bytes, cfg.band, name ? name : "device buffer", owner};
    g.nlive = (long)g.live.size();
    *p = inner;
    return hipSuccess;
}

// compares one band (len bytes at dev, whose first byte has offset off0 relative to the block) with the pattern; g.mu is held
inline int guard_check_band(GuardState &g, const GuardBlock &b, const char *dev, size_t len, long long off0, const char *side) {
    std::vector<unsigned char> host(len);
    if (hipMemcpy(host.data(), dev, len, hipMemcpyDeviceToHost) != hipSuccess) {
        g.log.push_back(b.name + ": " + side + " band could not be read back");
        return 1;
    }
    const size_t phase = (size_t)(off0 & 3);        // (off0 is a multiple of 4 in front, bytes behind)
    for (size_t i = 0; i < len; ++i) {
        if (host[i] == guard_band_byte(phase + i)) continue;
        const size_t w0 = (phase + i) / 4 * 4;      // the word that holds the byte, as far as it lies in this band
        uint32_t word = 0;
        for (size_t k = 0; k < 4; ++k) {
            const size_t at = w0 + k;
            const unsigned char c = at >= phase && at - phase < len ? host[at - phase] : guard_band_byte(at);
            word |= (uint32_t)c << (8 * k);
        }
        char text[256];
        snprintf(text, sizeof text, "%s: %s band, first differing byte at offset %lld of a block of %zu bytes, word 0x%08x",
                 b.name.c_str(), side, off0 + (long long)i, b.bytes, word);
        g.log.push_back(text);
        return 1;
    }
    return 0;
}

inline int guard_check_block(GuardState &g, const GuardBlock &b) {
    const char *inner = b.base + b.band;
    const size_t r4 = guard_round4(b.bytes);
    return guard_check_band(g, b, b.base, b.band, -(long long)b.band, "front") +
           guard_check_band(g, b, inner + b.bytes, r4 - b.bytes + b.band, (long long)b.bytes, "back");
}

// frees what guard_alloc returned, in any mode; a guarded block is checked first
inline void guard_free(void *p) {
    if (!p) return;
    GuardState &g = guard_state();
    if (g.nlive == 0) { hipFree(p); return; }
    std::lock_guard<std::mutex> lock(g.mu);
    auto it = g.live.find(p);
    if (it == g.live.end()) { hipFree(p); return; }
    hipDeviceSynchronize();
    guard_check_block(g, it->second);
    hipFree(it->second.base);
    g.live.erase(it);
    g.nlive = (long)g.live.size();
}

// every live block of one owner, without freeing; returns the number of violations it added to the log
inline int guard_check_owner(const void *owner) {
    GuardState &g = guard_state();
    if (g.nlive == 0) return 0;
    std::lock_guard<std::mutex> lock(g.mu);
    hipDeviceSynchronize();
    int bad = 0;
    for (const auto &kv : g.live)
        if (kv.second.owner == owner) bad += guard_check_block(g, kv.second);
    return bad;
}

// the log as text, one violation per line (truncated to n - 1 characters); returns the number of violations
inline int guard_report(char *buf, int n) {
    GuardState &g = guard_state();
    std::lock_guard<std::mutex> lock(g.mu);
    if (buf && n > 0) {
        std::string all;
        for (const std::string &s : g.log) { all += s; all += '\n'; }
        const size_t len = all.size() < (size_t)n - 1 ? all.size() : (size_t)n - 1;
        memcpy(buf, all.data(), len);
        buf[len] = 0;
    }
    return (int)g.log.size();
}

inline void guard_reset() {
    GuardState &g = guard_state();
    std::lock_guard<std::mutex> lock(g.mu);
    g.log.clear();
}
