// The host side of the far route (AFQ_THERMAL_FAR) as a stand-alone program for AddressSanitizer and UBSan
// (tests/test_thermal_far_sizes_cpu.py builds and runs it; no device is touched and no kernel is launched): the LDS and
// scratch size functions of thermal_wide.h, the bound they leave, and th_screen_bound with the far kernels on a handle
// that holds nothing but M.  One line per check: "ok <name>" or "FAIL <name>: <what>".
#include "../pauxy_amd/csrc/thermal_wide.h"
#include <cstdio>
#include <cstring>

static int failed = 0;

static void verdict(const char *name, bool ok, const std::string &what = "") {
    if (ok) printf("ok %s\n", name);
    else { printf("FAIL %s: %s\n", name, what.c_str()); failed = 1; }
}

static int screen(afq_handle *h, int M, const char *unit, const ThLds &slice) {
    h->M = M;
    h->err.clear();
    return th_screen_bound(h, "thermal walkers with continuous fields (far_basis)", unit, TW_COLS, false, {THC_FAR_GREENS, slice});
}

int main() {
    // the vectors alone: 18,944 B for cplx whatever M is; half of them for double but the int perm
    bool ok = true;
    for (int M = 1; M <= 4096; ++M)
        ok = ok && ts_greens_far_lds<cplx>(M) == 18944 && ts_greens_far_lds<double>(M) == 8 * 1152 + 512 && thc_slice_far_lds(M) == 0 &&
             thd_slice_far_lds(M) == 2048;
    verdict("lds-is-the-vectors", ok);
    verdict("lds-is-the-wide-kernels-less-its-matrix", ts_greens_wide_lds<cplx>(93) - 16 * ts_mat(93) == ts_greens_far_lds<cplx>(93));

    // scratch: four [M, M] and W [M, M | 1] behind them, in scalars; no overflow of the byte count at any M an int holds
    ok = true;
    for (int M = 1; M <= 128; ++M) {
        const size_t want = 4 * (size_t)M * M + (size_t)M * (M | 1);
        ok = ok && ts_greens_far_scratch(M) == want && ts_greens_far_scratch(M) == ts_greens_wide_scratch(M) + ts_mat(M);
    }
    verdict("scratch-is-four-buffers-and-w", ok);
    verdict("scratch-at-123", ts_greens_far_scratch(123) == 4 * 15129 + 123 * 123 && ts_greens_far_scratch(128) == 4 * 16384 + 128 * 129);
    const size_t big = ts_greens_far_scratch(46340);                 // (M M still fits an int; the product must not wrap)
    verdict("scratch-in-size_t", big == 4 * (size_t)46340 * 46340 + (size_t)46340 * 46341 && big * 16 > big);
    // a population's bytes at the bound: 2 work-groups per walker
    verdict("scratch-bytes-of-256-walkers", 2 * ts_greens_far_scratch(128) * 256 * 16 == (size_t)256 * 2 * (65536 + 16512) * 16);

    verdict("bound-is-128", th_far_bound() == 128 && th_far_bound() == TW_COLS);

    afq_handle *h = new afq_handle();
    ok = true;
    for (int M = 1; M <= 128; ++M) ok = ok && screen(h, M, "sites", THD_FAR_SLICE) == AFQ_OK && h->err.empty();
    verdict("screen-passes-to-128", ok);
    int rc = screen(h, 129, "sites", THD_FAR_SLICE);
    verdict("screen-refuses-129-sites", rc == AFQ_EUNSUPPORTED &&
            h->err == "thermal walkers with continuous fields (far_basis): M = 129 sites are more than the 128 columns of a wave, "
                      "two per lane (M <= 128)", h->err);
    rc = screen(h, 171, "plane waves", THC_FAR_SLICE);
    verdict("screen-refuses-171-plane-waves", rc == AFQ_EUNSUPPORTED && h->err.find("M = 171 plane waves") != std::string::npos &&
            h->err.find("(M <= 128)") != std::string::npos, h->err);
    rc = screen(h, 1000000, "sites", THD_FAR_SLICE);
    verdict("screen-refuses-a-million", rc == AFQ_EUNSUPPORTED && h->err.find("(M <= 128)") != std::string::npos, h->err);
    // the wide kernels under the same screen: the first that does not fit is named with its bytes
    h->M = 96; h->err.clear();
    rc = th_screen_bound(h, "w", "sites", TW_COLS, false, {{"the wide Green's function", ts_greens_wide_lds<cplx>, ""}});
    verdict("screen-names-bytes-of-a-kernel-that-does-not-fit", rc == AFQ_EUNSUPPORTED && h->err.find("167936") != std::string::npos &&
            h->err.find("(M <= 95)") != std::string::npos, h->err);
    delete h;
    return failed;
}
