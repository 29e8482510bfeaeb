// Imaginary-time single-particle Green's function (estimators/itcf.py of the reference, DESIGN row 8f-3): the
// explicit propagator matrices B_t of a walker's recorded fields, their inverses, the per-slice products of the
// stable and unstable chains and the weighted walker sums.  The window itself is driven by afq_itcf_update.
//
// Every product is a batched complex M x M (or M x N) GEMM on the per-wave fp64 MFMA engine of mfma_gemm.h; the
// inverses of the Generic exponentials go through the register-resident Gauss-Jordan kernel of k_bigdet.hip (M <= 128).
#include "afq_internal.h"
#include "mfma_gemm.h"

namespace {

// C[b] = alpha * A'[b] B[b] + diag * I with batch b = w * nsp + s and A'(r, k) = A[b](r, k) (* sc[b][k] when sc is set):
// every operand addressed as base + w * (w stride) + s * (s stride), so a stride of 0 shares a matrix (BT2 over the
// walkers, the exponential over the spins)
struct ItcfGemm {
    static constexpr bool A_CPLX = true, B_CPLX = true;
    int batch, rows, cols, kdim, nsp;
    const cplx *A; long aw, as; int lda;
    const double *sc; long sw, ss;
    const cplx *B; long bw, bs; int ldb;
    cplx *C; long cw, cs; int ldc;
    double alpha, diag;
    __device__ bool active(int) const { return true; }
    __device__ cplx loadA(int b, int r, int k) const {
        const long w = b / nsp, s = b % nsp;
        const cplx v = A[w * aw + s * as + (long)r * lda + k];
        return sc ? cscale(v, sc[w * sw + s * ss + k]) : v;
    }
    __device__ cplx loadB(int b, int k, int c) const {
        const long w = b / nsp, s = b % nsp;
        return B[w * bw + s * bs + (long)k * ldb + c];
    }
    __device__ void store(int b, int r, int c, double re, double im) const {
        const long w = b / nsp, s = b % nsp;
        C[w * cw + s * cs + (long)r * ldc + c] = cmake(alpha * re + (r == c ? diag : 0.0), alpha * im);
    }
};

// dst[w][:, spin s columns] = Bm[w, s] src[w][:, spin s columns]; batch b = 2 w + s, cols = max(na, nb)
struct ItcfPsiProp {
    static constexpr bool A_CPLX = true, B_CPLX = true;
    int batch, rows, cols, kdim;
    const cplx *Bm;
    const cplx *src;
    cplx *dst;
    int M, nt, na, nb;
    __device__ bool active(int) const { return true; }
    __device__ cplx loadA(int b, int r, int k) const { return Bm[(long)b * M * M + (long)r * M + k]; }
    __device__ cplx loadB(int b, int k, int c) const {
        const int s = b & 1;
        if (c >= (s ? nb : na)) return cmake(0.0, 0.0);
        return src[(long)(b >> 1) * M * nt + (long)k * nt + (s ? na : 0) + c];
    }
    __device__ void store(int b, int r, int c, double re, double im) const {
        const int s = b & 1;
        if (c < (s ? nb : na)) dst[(long)(b >> 1) * M * nt + (long)r * nt + (s ? na : 0) + c] = cmake(re, im);
    }
};

template <class P> int run_gemm(afq_handle *h, const P &p) {
    // 32 x 32 output blocks per wave: at M = 100 a (walker, spin) batch is 16 wave tasks
    AFQ_GEMM(h, (launch_mfma_gemm<2, 2, P>(p, h->stream)));
    return AFQ_OK;
}

ItcfGemm gemm(int batch, int nsp, int n, int m, int k) {
    ItcfGemm p;
    p.batch = batch * nsp; p.nsp = nsp; p.rows = n; p.cols = m; p.kdim = k;
    p.sc = nullptr; p.sw = p.ss = 0; p.alpha = 1.0; p.diag = 0.0;
    return p;
}

}   // namespace

// recorded fields of window step t for every walker: xs[w] = hist[w, t]
__global__ void itcf_fields_kernel(const cplx *hist, cplx *xs, int K, int nbp, int t) {
    const int w = blockIdx.x;
    const cplx *src = hist + ((long)w * nbp + t) * K;
    for (int k = threadIdx.x; k < K; k += blockDim.x) xs[(long)w * K + k] = src[k];
}

// discrete fields of window step t: f[w, s, j] = auxf[x_j, s] and its reciprocal (propagation/hubbard.py:589-593)
__global__ void itcf_hirsch_diag_kernel(const cplx *hist, double *f, double *finv, int nw, int M, int nbp, int t,
                                        double eg, double emg) {
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (e >= 2L * nw * M) return;
    const int j = (int)(e % M), s = (int)((e / M) % 2);
    const long w = e / (2L * M);
    const int x = (int)hist[(w * nbp + t) * M + j].x;
    const bool up = s == 0;
    const double v = (x == 0) == up ? eg : emg;
    f[e] = v;
    finv[e] = 1.0 / v;
}

// Horner start of the order-6 Taylor series: X = I + V / 6
__global__ void itcf_taylor_start_kernel(const cplx *V, cplx *X, long n, int M) {
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int r = (int)((e / M) % M), c = (int)(e % M);
    const cplx v = V[e];
    X[e] = cmake(v.x / 6.0 + (r == c ? 1.0 : 0.0), v.y / 6.0);
}

// P = G^T (the device's G holds gab(psi_L, psi_R)^T per spin), Q = I - P
__global__ void itcf_projectors_kernel(const cplx *G, cplx *P, cplx *Q, long n, int M) {
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (e >= n) return;
    const long mat = e / ((long)M * M);
    const int r = (int)((e / M) % M), c = (int)(e % M);
    const cplx g = G[mat * M * M + (long)c * M + r];
    P[e] = g;
    Q[e] = cmake((r == c ? 1.0 : 0.0) - g.x, -g.y);
}

// wfac_w (0 for walkers without a complete window) and denom += sum_w wfac_w
__global__ void itcf_weights_kernel(const double *weight, const double *bp_cos, const cplx *bp_ph, const int *bp_n,
                                    int need, int restore, int nw, cplx *wfac, cplx *denom) {
    __shared__ cplx part[256];
    cplx acc = cmake(0.0, 0.0);
    for (int w = threadIdx.x; w < nw; w += blockDim.x) {
        cplx v = cmake(bp_n[w] >= need ? weight[w] : 0.0, 0.0);
        if (restore && v.x != 0.0) v = cmul(v, cmake(bp_ph[w].x / bp_cos[w], bp_ph[w].y / bp_cos[w]));
        wfac[w] = v;
        acc = cadd(acc, v);
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] = cadd(part[threadIdx.x], part[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *denom = cadd(*denom, part[0]);
}

// spgf[tau, s, 0] += sum_w wfac_w Re Ggr[w, s], spgf[tau, s, 1] += sum_w wfac_w Re Gls[w, s] (itcf.py accumulate_uhf);
// walkers with wfac 0 are skipped, so that a dead walker's matrices never enter the sums
__global__ void itcf_accumulate_kernel(const cplx *Ggr, const cplx *Gls, const cplx *wfac, cplx *spgf, int nw, int M) {
    const long mm = (long)M * M;
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (e >= 4 * mm) return;
    const int s = (int)(e / (2 * mm)), g = (int)((e / mm) % 2);
    const long ij = e % mm;
    const cplx *src = g ? Gls : Ggr;
    cplx acc = cmake(0.0, 0.0);
    for (int w = 0; w < nw; ++w) {
        const cplx wt = wfac[w];
        if (wt.x == 0.0 && wt.y == 0.0) continue;
        const double re = src[((long)w * 2 + s) * mm + ij].x;
        acc = cmake(acc.x + wt.x * re, acc.y + wt.y * re);
    }
    spgf[e] = cadd(spgf[e], acc);
}

int k_itcf_fields(afq_handle *h, cplx *xs, int t) {
    AFQ_LAUNCH(h, itcf_fields_kernel, dim3(h->nw), dim3(128), 0, h->stream, h->bp_hist, xs, h->K, h->nbp, t);
    AFQ_POST(h);
    return AFQ_OK;
}

// B[w, s] = BT2_s E[w] BT2_s with E = sum_{k <= 6} V^k / k! of V = vhs[w] (propagation/generic.py:181-207), and
// Binv[w, s] = BT2_s^-1 E[w]^-1 BT2_s^-1.  ws: 2 [nw, M, M] + 2 [nw, 2, M, M] of scratch.
int k_itcf_generic_b(afq_handle *h, const cplx *vhs, const cplx *BT2, const cplx *BT2inv, cplx *B, cplx *Binv, cplx *ws,
                     cplx *detm, int *dete) {
    const int M = h->M, nw = h->nw;
    const long mm = (long)M * M, n1 = (long)nw * mm;
    cplx *X0 = ws, *X1 = ws + n1, *T = ws + 2 * n1;
    AFQ_LAUNCH(h, itcf_taylor_start_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, h->stream, vhs, X0, n1, M);
    AFQ_POST(h);
    int rc;
    for (int k = 5; k >= 1; --k) {                               // X <- I + V X / k
        ItcfGemm p = gemm(nw, 1, M, M, M);
        p.A = vhs; p.aw = mm; p.as = 0; p.lda = M;
        p.B = X0; p.bw = mm; p.bs = 0; p.ldb = M;
        p.C = X1; p.cw = mm; p.cs = 0; p.ldc = M;
        p.alpha = 1.0 / k; p.diag = 1.0;
        if ((rc = run_gemm(h, p))) return rc;
        std::swap(X0, X1);
    }
    // X0 = E; X1 <- E^-1 (in place Gauss-Jordan on a copy)
    AFQ_HIP(h, hipMemcpyAsync(X1, X0, sizeof(cplx) * n1, hipMemcpyDeviceToDevice, h->stream));
    if ((rc = k_gj_inverse(h, X1, M, nw, detm, dete))) return rc;
    const cplx *E[2] = {X0, X1}, *R[2] = {BT2, BT2inv};
    cplx *out[2] = {B, Binv};
    for (int q = 0; q < 2; ++q) {
        ItcfGemm p = gemm(nw, 2, M, M, M);                       // T[w, s] = E[w] R_s
        p.A = E[q]; p.aw = mm; p.as = 0; p.lda = M;
        p.B = R[q]; p.bw = 0; p.bs = mm; p.ldb = M;
        p.C = T; p.cw = 2 * mm; p.cs = mm; p.ldc = M;
        if ((rc = run_gemm(h, p))) return rc;
        ItcfGemm r = gemm(nw, 2, M, M, M);                       // out[w, s] = R_s T[w, s]
        r.A = R[q]; r.aw = 0; r.as = mm; r.lda = M;
        r.B = T; r.bw = 2 * mm; r.bs = mm; r.ldb = M;
        r.C = out[q]; r.cw = 2 * mm; r.cs = mm; r.ldc = M;
        if ((rc = run_gemm(h, r))) return rc;
    }
    return AFQ_OK;
}

// B[w, s] = BT2_s diag(auxf[x_t, s]) BT2_s (propagation/hubbard.py:568-600) and Binv = BT2_s^-1 diag(1 / auxf) BT2_s^-1
// for the discrete fields of window step t.  f: 2 [nw, 2, M] doubles of scratch.
int k_itcf_hirsch_b(afq_handle *h, int t, const cplx *BT2, const cplx *BT2inv, cplx *B, cplx *Binv, double *f) {
    const int M = h->M, nw = h->nw;
    const long mm = (long)M * M, nf = 2L * nw * M;
    const double g = acosh(exp(0.5 * h->dt * h->U));
    AFQ_LAUNCH(h, itcf_hirsch_diag_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, h->stream, h->bp_hist,
               f, f + nf, nw, M, h->nbp, t, exp(g), exp(-g));
    AFQ_POST(h);
    const cplx *R[2] = {BT2, BT2inv};
    cplx *out[2] = {B, Binv};
    for (int q = 0; q < 2; ++q) {
        ItcfGemm p = gemm(nw, 2, M, M, M);
        p.A = R[q]; p.aw = 0; p.as = mm; p.lda = M;
        p.sc = f + q * nf; p.sw = 2L * M; p.ss = M;
        p.B = R[q]; p.bw = 0; p.bs = mm; p.ldb = M;
        p.C = out[q]; p.cw = 2 * mm; p.cs = mm; p.ldc = M;
        const int rc = run_gemm(h, p);
        if (rc) return rc;
    }
    return AFQ_OK;
}

// C[w, s] = A[w, s] B[w, s] for [nw, 2, M, M] operands
int k_itcf_mul(afq_handle *h, const cplx *A, const cplx *B, cplx *C) {
    const int M = h->M;
    const long mm = (long)M * M;
    ItcfGemm p = gemm(h->nw, 2, M, M, M);
    p.A = A; p.aw = 2 * mm; p.as = mm; p.lda = M;
    p.B = B; p.bw = 2 * mm; p.bs = mm; p.ldb = M;
    p.C = C; p.cw = 2 * mm; p.cs = mm; p.ldc = M;
    return run_gemm(h, p);
}

// dst[w] = B[w, s] src[w] per spin block of columns
int k_itcf_propagate(afq_handle *h, const cplx *B, const cplx *src, cplx *dst) {
    ItcfPsiProp p;
    p.batch = 2 * h->nw; p.rows = h->M; p.cols = h->na > h->nb ? h->na : h->nb; p.kdim = h->M;
    p.Bm = B; p.src = src; p.dst = dst; p.M = h->M; p.nt = h->nt; p.na = h->na; p.nb = h->nb;
    if (p.cols == 0) return AFQ_OK;
    return run_gemm(h, p);
}

int k_itcf_projectors(afq_handle *h, const cplx *G, cplx *P, cplx *Q) {
    const long n = 2L * h->nw * h->M * h->M;
    AFQ_LAUNCH(h, itcf_projectors_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, G, P, Q, n, h->M);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_itcf_weights(afq_handle *h, int restore, cplx *wfac, cplx *denom) {
    const int need = h->nbp * (h->hirsch ? h->M : 1);          // discrete fields: bp_n counts single fields
    AFQ_LAUNCH(h, itcf_weights_kernel, dim3(1), dim3(256), 0, h->stream, h->weight, h->bp_cos, h->bp_ph, h->bp_n, need,
               restore, h->nw, wfac, denom);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_itcf_accumulate(afq_handle *h, const cplx *Ggr, const cplx *Gls, const cplx *wfac, cplx *spgf_tau) {
    const long n = 4L * h->M * h->M;
    AFQ_LAUNCH(h, itcf_accumulate_kernel, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, h->stream, Ggr, Gls, wfac,
               spgf_tau, h->nw, h->M);
    AFQ_POST(h);
    return AFQ_OK;
}
