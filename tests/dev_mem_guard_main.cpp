// The guard mode of the handle's device memory (pauxy_amd/csrc/dev_guard.h, dev_mem.h) on the host alone, over the shim of
// tests/dev_mem_shim.h: every check prints "ok <name>" or "FAIL <name>: <why>"; tests/test_dev_mem_guard_cpu.py builds this
// under AddressSanitizer and UBSan and holds the output to the list of checks.
#include <cmath>
#include <cstdio>
#include <string>
#include "../pauxy_amd/csrc/dev_mem.h"

struct cplx { double x, y; };
template <> struct DevFloating<cplx> : std::true_type {};

static int failures = 0;
static void verdict(const char *name, bool ok, const std::string &why = "") {
    if (ok) printf("ok %s\n", name);
    else { printf("FAIL %s: %s\n", name, why.c_str()); ++failures; }
}

static std::string report(int *count = nullptr) {
    char buf[4096];
    const int n = guard_report(buf, sizeof buf);
    if (count) *count = n;
    return buf;
}

static DevMem mem_of(int mode, size_t band = 4096) {
    DevMem m;
    m.guard.mode = mode; m.guard.band = band;
    return m;
}

// one block of `bytes` named "alpha"; poke writes outside it; the violation must surface at `when` with the text `expect`
enum When { AT_CHECK, AT_REPLACE, AT_RELEASE };
template <class Poke> static void poked(const char *name, int mode, size_t bytes, Poke poke, When when, const std::string &expect) {
    guard_reset();
    DevMem m = mem_of(mode);
    char *alpha = nullptr, *beta = nullptr;
    m.replace(LT_WALKERS, (void **)&alpha, bytes, nullptr, false, "alpha");
    m.replace(LT_WALKERS, (void **)&beta, 64, nullptr, false, "beta");
    poke(alpha);
    int n = 0;
    if (when == AT_CHECK) {
        const int bad = guard_check_owner(&m);
        report(&n);
        if (bad != 1 || n != 1) { verdict(name, false, "check found " + std::to_string(bad)); m.release(LT_WALKERS); return; }
    }
    if (when == AT_REPLACE) m.replace(LT_WALKERS, (void **)&alpha, 2 * bytes, nullptr, false, "alpha");     // the dev_grow case
    if (when != AT_CHECK) report(&n);
    if (when == AT_REPLACE && n != 1) { verdict(name, false, "replace logged " + std::to_string(n)); m.release(LT_WALKERS); return; }
    if (when == AT_CHECK) guard_reset();
    m.release(LT_WALKERS);
    const std::string text = report(&n);
    verdict(name, n == 1 && text == expect + "\n" && alpha == nullptr && beta == nullptr, text);
}

static std::string line(const char *side, long long off, size_t bytes, unsigned word) {
    char t[256];
    snprintf(t, sizeof t, "alpha: %s band, first differing byte at offset %lld of a block of %zu bytes, word 0x%08x", side, off, bytes, word);
    return t;
}

int main() {
    int n = 0;
    // ---- untouched blocks pass, modes 1 and 2, through replace, release and the check without freeing
    for (int mode = 1; mode <= 2; ++mode) {
        guard_reset();
        DevMem m = mem_of(mode);
        double *a = nullptr; int *b = nullptr; char *c = nullptr;
        size_t len = 7;
        m.replace(LT_WALKERS, (void **)&a, 24 * sizeof(double), &len, true, "a");
        m.replace(LT_SYSTEM, (void **)&b, 5 * sizeof(int), nullptr, false, "b");
        m.replace(LT_WALKERS, (void **)&c, 13, nullptr, false, "c");
        const bool aligned = (uintptr_t)a % 4096 == 0 && (uintptr_t)b % 4096 == 0 && (uintptr_t)c % 4096 == 0;
        bool body = true;
        if (mode == 2) {
            for (int i = 0; i < 24; ++i) body = body && std::isnan(a[i]) && std::isnan(((float *)a)[2 * i]) && std::isnan(((float *)a)[2 * i + 1]);
            for (int i = 0; i < 5; ++i) body = body && b[i] == 0;
            for (int i = 0; i < 13; ++i) body = body && c[i] == 0;
        }
        for (int i = 0; i < 24; ++i) a[i] = i;          // the whole body is the caller's
        for (int i = 0; i < 5; ++i) b[i] = i;
        for (int i = 0; i < 13; ++i) c[i] = (char)i;
        const int bad = guard_check_owner(&m);
        m.replace(LT_WALKERS, (void **)&a, 48 * sizeof(double), &len, true, "a");
        for (int i = 0; i < 48; ++i) a[i] = i;
        m.release(LT_WALKERS); m.release(LT_SYSTEM);
        report(&n);
        verdict(mode == 1 ? "untouched-mode1" : "untouched-mode2", bad == 0 && n == 0 && !a && !b && !c && len == 0 && m.allocations == 4, report());
        verdict(mode == 1 ? "aligned-mode1" : "aligned-mode2", aligned);
        if (mode == 2) verdict("poison-typed", body);
    }
    // ---- single bytes in the bands, and a complex store one element past the end
    const size_t B = 48, band = 4096;
    poked("byte-before", 1, B, [](char *p) { p[-1] = 0x55; }, AT_CHECK, line("front", -1, B, 0x55f8beefu));
    poked("byte-behind", 1, B, [&](char *p) { p[B] = 0x55; }, AT_CHECK, line("back", B, B, 0x7ff8be55u));
    poked("byte-front-far", 2, B, [&](char *p) { p[-(long)band] = 0x55; }, AT_CHECK, line("front", -(long long)band, B, 0x7ff8be55u));
    poked("byte-back-far", 2, B, [&](char *p) { p[B + band - 1] = 0x55; }, AT_CHECK, line("back", B + band - 1, B, 0x55f8beefu));
    poked("byte-behind-odd-size", 1, 13, [](char *p) { p[13] = 0x55; }, AT_CHECK, line("back", 13, 13, 0x7ff855efu));
    poked("byte-back-far-odd-size", 1, 13, [&](char *p) { p[16 + band - 1] = 0x55; }, AT_CHECK, line("back", 16 + band - 1, 13, 0x55f8beefu));
    poked("complex-store-past-end", 1, 3 * sizeof(cplx), [](char *p) { ((cplx *)p)[3] = cplx{1.0, 2.0}; }, AT_CHECK, line("back", 48, 48, 0x00000000u));
    // ---- where a band write surfaces without an explicit check
    poked("reported-at-replace", 1, B, [&](char *p) { p[B + 7] = 1; }, AT_REPLACE, line("back", B + 7, B, 0x01f8beefu));
    poked("reported-at-release", 1, B, [](char *p) { p[-8] = 1; }, AT_RELEASE, line("front", -8, B, 0x7ff8be01u));
    {
        guard_reset();
        DevMem m = mem_of(2);
        bool nan = true;
        {
            DevTemp<double> t;
            t.alloc(9, &m, "gamma");
            for (int i = 0; i < 9; ++i) nan = nan && std::isnan(t.p[i]);
            nan = nan && (uintptr_t)t.p % 4096 == 0;
            t.p[9] = 3.0;
        }
        const std::string text = report(&n);
        verdict("reported-at-scope-exit", nan && n == 1 && text == "gamma: back band, first differing byte at offset 72 of a block of 72 bytes, word 0x00000000\n", text);
        guard_reset();
        { DevTemp<cplx> t; t.alloc(4, &m); for (int i = 0; i < 4; ++i) t.p[i] = cplx{0.0, 0.0}; }
        report(&n);
        verdict("devtemp-untouched", n == 0, report());
    }
    // ---- mode 0: the requested bytes, the allocator's pointer, no registry, no synchronisation, no log
    {
        guard_reset();
        const size_t syncs = shim_syncs, mallocs = shim_mallocs, frees = shim_frees;
        DevMem m = mem_of(0);
        char *a = nullptr;
        m.replace(LT_WALKERS, (void **)&a, 13, nullptr, false, "a");
        bool ok = shim_last_bytes == 13 && shim_last_ptr == a && guard_state().nlive == 0;
        for (int i = 0; i < 13; ++i) a[i] = 1;
        { DevTemp<double> t; t.alloc(3); ok = ok && shim_last_bytes == 24 && shim_last_ptr == t.p; }
        { DevTemp<double> t; t.alloc(3, &m); ok = ok && shim_last_bytes == 24 && shim_last_ptr == t.p; }
        ok = ok && guard_check_owner(&m) == 0;
        m.release(LT_WALKERS);
        report(&n);
        verdict("mode0-exact", ok && n == 0 && !a && shim_syncs == syncs && shim_mallocs == mallocs + 3 && shim_frees == frees + 3);
    }
    // ---- the environment: the mode, and a band rounded up to whole pages
    {
        setenv("AFQ_DEBUG_GUARD", "2", 1); setenv("AFQ_DEBUG_GUARD_BYTES", "65000", 1);
        const GuardCfg c = guard_cfg_from_env();
        setenv("AFQ_DEBUG_GUARD", "0", 1); unsetenv("AFQ_DEBUG_GUARD_BYTES");
        const GuardCfg z = guard_cfg_from_env();
        unsetenv("AFQ_DEBUG_GUARD");
        const GuardCfg u = guard_cfg_from_env();
        verdict("environment", c.mode == 2 && c.band == 65536 && z.mode == 0 && z.band == 4096 && u.mode == 0);
    }
    verdict("nothing-left-live", guard_state().nlive == 0 && shim_mallocs == shim_frees);
    return failures ? 1 : 0;
}
