// The host side of the quad route (AFQ_THERMAL_QUAD) as a stand-alone program for AddressSanitizer and UBSan
// (tests/test_thermal_quad_sizes_cpu.py builds and runs it; no device is touched and no kernel is launched): the quad LDS
// and scratch size functions of thermal_wide.h, the bound they leave, and th_screen_bound with the quad kernels -- and,
// unchanged, with TW_COLS -- on a handle that holds nothing but M.  One line per check: "ok <name>" or "FAIL <name>: <what>".
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
    return th_screen_bound(h, "thermal walkers with continuous fields (quad_basis)", unit, TQ_COLS, false, {THC_QUAD_GREENS, slice});
}

int main() {
    // the vectors alone at 256 columns: D, v, 4 of part, 3 of aux, and perm -- 37,888 B for cplx whatever M is
    bool ok = true;
    for (int M = 1; M <= 4096; ++M)
        ok = ok && ts_greens_quad_lds<cplx>(M) == 16 * 9 * 256 + 4 * 256 && ts_greens_quad_lds<cplx>(M) == 37888 &&
             thc_slice_quad_lds(M) == 0 && thd_slice_quad_lds(M) == 4096;
    verdict("lds-is-the-vectors-at-256", ok);
    verdict("lds-is-twice-the-far-kernels", ts_greens_quad_lds<cplx>(200) == 2 * ts_greens_far_lds<cplx>(200) &&
            thd_slice_quad_lds(200) == 2 * thd_slice_far_lds(200) && TQ_COLS == 2 * TW_COLS);
    verdict("lds-fits-a-work-group", ts_greens_quad_lds<cplx>(256) <= TH_LDS_MAX && thd_slice_quad_lds(256) <= TH_LDS_MAX);

    // scratch: the far route's, four [M, M] and W [M, M | 1] behind them, in scalars
    ok = true;
    for (int M = 1; M <= 256; ++M) ok = ok && TsQuad<cplx>::scratch(M) == 4 * (size_t)M * M + (size_t)M * (M | 1) && TsQuad<cplx>::scratch(M) == ts_greens_far_scratch(M);
    verdict("scratch-is-the-far-routes", ok);
    verdict("scratch-at-147-and-256", TsQuad<cplx>::scratch(147) == 4 * 21609 + 147 * 147 && TsQuad<cplx>::scratch(256) == 4 * 65536 + 256 * 257);
    // a population's bytes at the bound, 2 work-groups per walker: 2.7 GB, beyond 32 bits
    const size_t bytes = 2 * TsQuad<cplx>::scratch(256) * 256 * 16;
    verdict("scratch-bytes-of-256-walkers-in-size_t", bytes == (size_t)256 * 2 * (4 * 65536 + 256 * 257) * 16 && bytes == 2686451712ull &&
            bytes > 0xffffffffull / 2, std::to_string(bytes));

    verdict("bound-is-256", th_quad_bound() == 256 && th_quad_bound() == TQ_COLS);
    verdict("far-bound-is-still-128", th_far_bound() == 128 && TW_COLS == 128);

    afq_handle *h = new afq_handle();
    ok = true;
    for (int M = 1; M <= 256; ++M) ok = ok && screen(h, M, "sites", THD_QUAD_SLICE) == AFQ_OK && h->err.empty();
    verdict("screen-passes-to-256", ok);
    int rc = screen(h, 257, "sites", THD_QUAD_SLICE);
    verdict("screen-refuses-257-sites", rc == AFQ_EUNSUPPORTED &&
            h->err == "thermal walkers with continuous fields (quad_basis): M = 257 sites are more than the 256 columns of a wave, "
                      "four per lane (M <= 256)", h->err);
    rc = screen(h, 305, "plane waves", THC_QUAD_SLICE);
    verdict("screen-refuses-305-plane-waves", rc == AFQ_EUNSUPPORTED && h->err.find("M = 305 plane waves") != std::string::npos &&
            h->err.find("256 columns of a wave, four per lane") != std::string::npos && h->err.find("(M <= 256)") != std::string::npos, h->err);
    rc = screen(h, 1000000, "sites", THD_QUAD_SLICE);
    verdict("screen-refuses-a-million", rc == AFQ_EUNSUPPORTED && h->err.find("(M <= 256)") != std::string::npos, h->err);
    // TW_COLS and 64 lanes under the same screen: worded as before
    h->M = 129; h->err.clear();
    rc = th_screen_bound(h, "w", "sites", TW_COLS, false, {THC_FAR_GREENS, THD_FAR_SLICE});
    verdict("screen-words-128-columns-as-before", rc == AFQ_EUNSUPPORTED &&
            h->err == "w: M = 129 sites are more than the 128 columns of a wave, two per lane (M <= 128)", h->err);
    h->M = 65; h->err.clear();
    rc = th_screen_bound(h, "w", "sites", 64, true, {});
    verdict("screen-words-64-lanes-as-before", rc == AFQ_EUNSUPPORTED &&
            h->err == "w: M = 65 sites are more than the 64 lanes of a wave, one per column (M <= 64)", h->err);
    delete h;
    return failed;
}
