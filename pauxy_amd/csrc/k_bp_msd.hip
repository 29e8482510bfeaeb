// Back-propagation of a multi-determinant trial |psi_T> = sum_d c_d |D_d> (afq_bp_update_msd, DESIGN row 8f-2):
//   the backward pass D_d <- B(x)^H D_d of every determinant of a walker over ONE HS potential per walker and step,
//   the relative normalisation log r_d the re-orthogonalisations leave behind, the weights
//   w_d = conj(c_d) exp(log r_d - max log r) <Q_d|phi_old> and the determinant-weighted sums.
//
// phi_bp is [ndet, nw, M, nt]: slab d is an ordinary population of nw walkers for the re-orthogonalisation, the
// overlap and the Green's function kernels.  On the GEMM chain (no fused propagator for the shape) the ndet
// determinants of a walker are the columns of one stacked operand [M, ndet nt]: column c of walker w is column
// c % ns of determinant c / ns, so that BH1^H and the walker's V are streamed once per product for ndet times the
// columns.  That is addressing alone (StackMap); the engines are those of k_gemm.hip with problem types of their own,
// so the forward step's instantiations are not touched.
#include "mfma_gemm_wg.h"

namespace {

// column `col` of walker b's stacked operand: ns columns per determinant in this launch, the first of them column
// `off` of the determinant's nt
struct StackMap {
    int ns, off, nt;
    long dstride, per;               // elements between determinants (nw M nt) and between walkers (M nt)
    __device__ long at(int b, int col) const {
        const int d = col / ns;
        return d * dstride + (long)b * per + off + (col - d * ns);
    }
};

template <bool AR>
struct OneBodyStackProbT {
    static constexpr bool A_CPLX = true, B_CPLX = true, A_REAL = AR;
    int batch, rows, cols, kdim;     // nw, M, ndet ns, M
    StackMap m;
    const cplx *B1;                  // BH1^H[s]  [M, M]
    const cplx *src;                 // [ndet, nw, M, nt]
    cplx *dst;
    const int *alive;
    __device__ bool active(int b) const { return alive[b] != 0; }
    // walkers whose history has run out are not propagated, and source and destination differ: copied through
    static constexpr bool INACTIVE_COPY = true;
    __device__ void inactive_tile(int b, int row0, int nr, int col0, int nc, int t, int nthr) const {
        for (int e = t; e < nr * nc; e += nthr) {
            const int r = row0 + e / nc, c = col0 + e % nc;
            if (r < rows && c < cols) {
                const long idx = m.at(b, c) + (long)r * m.nt;
                dst[idx] = src[idx];
            }
        }
    }
    __device__ cplx loadA(int, int row, int k) const { return B1[(long)row * kdim + k]; }
    __device__ cplx loadB(int b, int k, int col) const { return src[m.at(b, col) + (long)k * m.nt]; }
    __device__ const cplx *ptrA(int, int row, int k) const { return B1 + (long)row * kdim + k; }
    __device__ const cplx *ptrB(int b, int k, int col) const { return src + m.at(b, col) + (long)k * m.nt; }
    static constexpr bool INCR = true;
    __device__ int klimit(int) const { return kdim; }
    __device__ const cplx *baseA(int, int row) const { return B1 + (long)row * kdim; }
    __device__ const cplx *baseB(int b, int col) const { return src + m.at(b, col); }
    __device__ long kstepA() const { return 1; }
    __device__ long kstepB(int) const { return m.nt; }
    __device__ bool rowok(int, int) const { return true; }
    __device__ bool colok(int, int) const { return true; }
    __device__ void store(int b, int row, int col, double re, double im) const {
        dst[m.at(b, col) + (long)row * m.nt] = cmake(re, im);
    }
};

// one Taylor term: tout = V tin / n, phi += tout, on the stacked columns; V indexed by the walker alone
struct TaylorStackProb {
    static constexpr bool A_CPLX = true, B_CPLX = true;
    int batch, rows, cols, kdim;     // nw, M, ndet nt, M
    StackMap m;
    long vstride;
    const cplx *vhs;                 // [nw, M, M]
    const cplx *tin;
    cplx *tout, *phi;
    double inv_n;
    const int *alive;
    __device__ bool active(int b) const { return alive[b] != 0; }
    __device__ cplx loadA(int b, int row, int k) const { return vhs[b * vstride + (long)row * kdim + k]; }
    __device__ cplx loadB(int b, int k, int col) const { return tin[m.at(b, col) + (long)k * m.nt]; }
    __device__ const cplx *ptrA(int b, int row, int k) const { return vhs + b * vstride + (long)row * kdim + k; }
    __device__ const cplx *ptrB(int b, int k, int col) const { return tin + m.at(b, col) + (long)k * m.nt; }
    static constexpr bool INCR = true;
    __device__ int klimit(int) const { return kdim; }
    __device__ const cplx *baseA(int b, int row) const { return vhs + b * vstride + (long)row * kdim; }
    __device__ const cplx *baseB(int b, int col) const { return tin + m.at(b, col); }
    __device__ long kstepA() const { return 1; }
    __device__ long kstepB(int) const { return m.nt; }
    __device__ bool rowok(int, int) const { return true; }
    __device__ bool colok(int, int) const { return true; }
    __device__ void store(int b, int row, int col, double re, double im) const {
        const long idx = m.at(b, col) + (long)row * m.nt;
        const cplx t = cmake(re * inv_n, im * inv_n);
        tout[idx] = t;
        const cplx o = phi[idx];
        phi[idx] = cmake(o.x + t.x, o.y + t.y);
    }
};

// the work-group ring engine for the shapes the forward chain gives it (M > 128, 64 or more walkers), else the
// per-wave register engine
bool ring_shape(const afq_handle *h, int cols) { return h->M > 128 && cols > 32 && h->nw >= 64; }

template <bool AR>
int onebody_stacked(afq_handle *h, int ndet, int s, const cplx *src, cplx *dst) {
    const int M = h->M;
    const int ns = s == 2 ? h->nt : s == 0 ? h->na : h->nb;
    OneBodyStackProbT<AR> p;
    p.batch = h->nw; p.rows = M; p.cols = ndet * ns; p.kdim = M;
    p.m.ns = ns; p.m.off = s == 1 ? h->na : 0; p.m.nt = h->nt;
    p.m.per = (long)M * h->nt; p.m.dstride = p.m.per * h->nw;
    p.B1 = h->BH1 + (long)(s == 1 ? 1 : 0) * M * M;
    p.src = src; p.dst = dst; p.alive = h->alive;
    if (ring_shape(h, p.cols)) {
        if constexpr (AR) AFQ_GEMM_AS(h, "k_bp_msd_onebody: stacked ring GEMM", (launch_mfma_gemm_wg<2, 2, 2, 2, 4, OneBodyStackProbT<AR>, MAP_COLS_FAST, true, 1, 3>(p, h->stream, h->zero_page)));
        else AFQ_GEMM_AS(h, "k_bp_msd_onebody: stacked ring GEMM", (launch_mfma_gemm_wg<2, 2, 2, 2, 4, OneBodyStackProbT<AR>, MAP_COLS_FAST, true, 1, 5, 4>(p, h->stream, h->zero_page)));
    } else {
        AFQ_GEMM_AS(h, "k_bp_msd_onebody: stacked GEMM", (launch_mfma_gemm<2, 2, OneBodyStackProbT<AR>, MAP_COLS_FAST>(p, h->stream, 4)));
    }
    return AFQ_OK;
}

}   // namespace

// dst[d, w][:, spin s] = BH1[s] src[d, w][:, spin s] for every determinant d of every walker with alive[w] set (BH1 is
// whatever the handle holds in that role: the backward pass lends it BH1^H); the others are copied through
int k_bp_msd_onebody(afq_handle *h, int ndet, const cplx *src, cplx *dst) {
    const bool merged = h->bh1_same && h->na > 0 && h->nb > 0;
    for (int s = merged ? 2 : 0; s < (merged ? 3 : 2); ++s) {
        if (s < 2 && (s == 0 ? h->na : h->nb) == 0) continue;
        const int rc = h->bh1_real ? onebody_stacked<true>(h, ndet, s, src, dst) : onebody_stacked<false>(h, ndet, s, src, dst);
        if (rc) return rc;
    }
    return AFQ_OK;
}

// phi <- sum_{n <= order} V[w]^n / n! phi on the stacked columns; t0 and t1 are term buffers of phi's size
int k_bp_msd_taylor(afq_handle *h, int ndet, const cplx *vhs, cplx *phi, cplx *t0, cplx *t1) {
    const int M = h->M;
    const long per = (long)M * h->nt;
    if (h->nv != 1 || h->vhs_diag) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "stacked Taylor products: one dense HS potential per walker");
    AFQ_HIP(h, hipMemcpyAsync(t0, phi, sizeof(cplx) * per * h->nw * ndet, hipMemcpyDeviceToDevice, h->stream));
    cplx *tin = t0, *tout = t1;
    for (int n = 1; n <= h->exp_order; ++n) {
        TaylorStackProb p;
        p.batch = h->nw; p.rows = M; p.kdim = M; p.cols = ndet * h->nt;
        p.m.ns = h->nt; p.m.off = 0; p.m.nt = h->nt; p.m.per = per; p.m.dstride = per * h->nw;
        p.vstride = (long)M * M; p.vhs = vhs;
        p.tin = tin; p.tout = tout; p.phi = phi; p.inv_n = 1.0 / n; p.alive = h->alive;
        if (ring_shape(h, p.cols))
            AFQ_GEMM_AS(h, "k_bp_msd_taylor: stacked ring GEMM", (launch_mfma_gemm_wg<2, 2, 2, 2, 4, TaylorStackProb, MAP_COLS_FAST, true, 1, 5, 4>(p, h->stream, h->zero_page)));
        else
            AFQ_GEMM_AS(h, "k_bp_msd_taylor: stacked GEMM", (launch_mfma_gemm<2, 2, TaylorStackProb, MAP_COLS_FAST>(p, h->stream, 4)));
        cplx *t = tin; tin = tout; tout = t;
    }
    return AFQ_OK;
}

// ---------------------------------------------------------------- relative normalisation and weighted sums
// log r_d += log det R of a re-orthogonalisation (det R = det R_alpha det R_beta > 0: the diagonals are norms)
__global__ void bp_msd_logr_kernel(const double *detR, double *logr, long n) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i < n) logr[i] += log(detR[i]);
}

// w_d = conj(c_d) exp(log r_d - max_d' log r_d') <Q_d|phi_old>, zero when not finite; S = sum_d w_d built up over the
// calls d = 0 .. ndet - 1.  logr, ovlp: [ndet, nw]; detw: [nw, ndet]
__global__ void bp_msd_detw_kernel(const cplx *coeffs, const double *logr, const cplx *ovlp, cplx *detw, cplx *S, int nw,
                                   int ndet, int d) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    double mx = -INFINITY;
    for (int dd = 0; dd < ndet; ++dd) {
        const double lr = logr[(long)dd * nw + w];
        if (lr > mx) mx = lr;
    }
    cplx wd = cmul(cconj(coeffs[d]), cscale(ovlp[(long)d * nw + w], exp(logr[(long)d * nw + w] - mx)));
    if (!(isfinite(wd.x) && isfinite(wd.y))) wd = cmake(0.0, 0.0);
    detw[(long)w * ndet + d] = wd;
    S[w] = d == 0 ? wd : cadd(S[w], wd);
}

// gsum[w] (+)= w_d G_d[w] and esum[w] (+)= w_d E_d[w]; d = 0 starts the sums
__global__ void bp_msd_gsum_kernel(const cplx *detw, const cplx *G, cplx *gsum, const cplx *E, cplx *esum, long gsz,
                                   int ndet, int d) {
    const int w = blockIdx.y;
    const cplx wd = detw[(long)w * ndet + d];
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (e < gsz) {
        const long i = (long)w * gsz + e;
        cplx acc = d == 0 ? cmake(0.0, 0.0) : gsum[i];
        cfma(acc, wd, G[i]);
        gsum[i] = acc;
    }
    if (E && e < 3) {
        cplx acc = d == 0 ? cmake(0.0, 0.0) : esum[3 * w + e];
        cfma(acc, wd, E[3 * w + e]);
        esum[3 * w + e] = acc;
    }
}

// per walker: the window's weight wt (bp_accumulate_kernel's), fac[w] = wt / S, fac[nw + w] = wt -- both zero for a
// walker that does not count (weight zero, S zero or not finite) -- and the weights normalised, detw[w, d] /= S
__global__ void bp_msd_finish_kernel(const double *weight, const double *bp_cos, const cplx *bp_ph, cplx *detw,
                                     const cplx *S, cplx *fac, int nw, int ndet, int restore) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    cplx wt = cmake(weight[w], 0.0);
    if (restore == 1) wt = cmul(wt, bp_ph[w]);
    else if (restore == 2) wt = cmul(wt, cmake(bp_ph[w].x / bp_cos[w], bp_ph[w].y / bp_cos[w]));
    const cplx s = S[w];
    const bool s_ok = isfinite(s.x) && isfinite(s.y) && (s.x != 0.0 || s.y != 0.0);
    const bool counts = s_ok && (wt.x != 0.0 || wt.y != 0.0);
    fac[w] = counts ? cdiv(wt, s) : cmake(0.0, 0.0);
    fac[nw + w] = counts ? wt : cmake(0.0, 0.0);
    for (int d = 0; d < ndet; ++d) {
        const long i = (long)w * ndet + d;
        detw[i] = s_ok ? cdiv(detw[i], s) : cmake(0.0, 0.0);
    }
}

// est[4 + e] += sum_w fac_w gsum[w, e], est[3] += sum_w wt_w, est[0:3] += sum_w fac_w esum[w] (the layout of
// bp_accumulate_kernel); walkers that do not count are skipped, whatever their sums hold
__global__ void bp_msd_accumulate_kernel(const cplx *gsum, const cplx *fac, const cplx *esum, cplx *est, int nw, long gsz) {
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (e > gsz + 3) return;
    if (e > gsz && !esum) return;
    cplx acc = cmake(0.0, 0.0);
    for (int w = 0; w < nw; ++w) {
        const cplx f = fac[w];
        if (f.x == 0.0 && f.y == 0.0) continue;
        if (e == gsz) acc = cadd(acc, fac[nw + w]);
        else if (e > gsz) cfma(acc, f, esum[3 * w + (e - gsz - 1)]);
        else cfma(acc, f, gsum[(long)w * gsz + e]);
    }
    if (e == gsz) est[3] = cadd(est[3], acc);
    else if (e > gsz) est[e - gsz - 1] = cadd(est[e - gsz - 1], acc);
    else est[4 + e] = cadd(est[4 + e], acc);
}

int k_bp_msd_logr(afq_handle *h, const double *detR, double *logr, long n) {
    AFQ_LAUNCH(h, bp_msd_logr_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, detR, logr, n);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_bp_msd_detw(afq_handle *h, int ndet, int d, const cplx *coeffs, const double *logr, const cplx *ovlp, cplx *detw,
                  cplx *S) {
    AFQ_LAUNCH(h, bp_msd_detw_kernel, dim3((h->nw + 127) / 128), dim3(128), 0, h->stream, coeffs, logr, ovlp, detw, S,
               h->nw, ndet, d);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_bp_msd_gsum(afq_handle *h, int ndet, int d, const cplx *detw, const cplx *G, cplx *gsum, const cplx *E, cplx *esum) {
    const long gsz = 2L * h->M * h->M;
    AFQ_LAUNCH(h, bp_msd_gsum_kernel, dim3((unsigned)((gsz + 255) / 256), h->nw), dim3(256), 0, h->stream, detw, G, gsum,
               E, esum, gsz, ndet, d);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_bp_msd_finish(afq_handle *h, int ndet, int restore, cplx *detw, const cplx *S, cplx *fac) {
    AFQ_LAUNCH(h, bp_msd_finish_kernel, dim3((h->nw + 127) / 128), dim3(128), 0, h->stream, h->weight, h->bp_cos,
               h->bp_ph, detw, S, fac, h->nw, ndet, restore);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_bp_msd_accumulate(afq_handle *h, const cplx *gsum, const cplx *fac, const cplx *esum, cplx *est) {
    const long gsz = 2L * h->M * h->M;
    AFQ_LAUNCH(h, bp_msd_accumulate_kernel, dim3((unsigned)((gsz + 4 + 127) / 128)), dim3(128), 0, h->stream, gsum, fac,
               esum, est, h->nw, gsz);
    AFQ_POST(h);
    return AFQ_OK;
}
