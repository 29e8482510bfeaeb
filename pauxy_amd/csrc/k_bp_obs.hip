// Back-propagated two-body RDM and EKT Fock matrices (estimators/back_propagation.py:168-175, estimators/ekt.py:10-73;
// DESIGN row 8f-2).  Every walker w contributes wt_w times a function of its back-propagated Green's function
// G_s = U_s V_s (U_s = conj(phi_bp)[:, spin s] M x N_s, V_s = the half-rotated G_bp, N_s x M), both of which
// afq_bp_update leaves behind (phi_bp's conjugate copy and ghalf).  All contractions run on the fp64 MFMA tile engine
// (mfma_gemm.h) through one strided-operand problem (BoGemm).
//
// EKT, per walker, in rank-N form (G^T = V^T U^T):
//   P_x = U^T L_x, Q_x = U^T L_x^T, R_x = V L_x, T_x = V_a L_x^T              [N x M] panels, chunks of x
//   W_x = P_x V^T  (X_s[x] = tr W_x),  W'_x(s) = T_x(a) U_s                   [N x N]
//   1p: sum_x G^T L_x G^T L_x^T - J terms = V^T sum_x (W_x + c_s[x] I) Q_x,   c_a = -2 X_b - X_a, c_b = -X_b
//   1h: sum_x G_a L_x^T G_s L_x - J terms = U_a sum_x [(W'_x(a) + c_a I) R_x(a) + W'_x(b) R_x(b)] + U_b sum_x c_b R_x(b)
// The closing products over (w, n) carry wt_w.  Terms linear in G are evaluated once per window on
// Gbar = sum_w wt_w G_w (the one-body sums of bp_est), the constant 2 I h1 scaled by sum_w wt_w.
//
// Two-body RDM: for every (p, q) one GEMM over the stacked contraction (3 nw) with walker-contiguous staging copies:
//   out[p,:,q,:] = A_p^T B_q - sum_s C_{s,q}^T D_{s,p},  A_p[w,r] = wt_w S_w[p,r], B_q[w,s] = S_w[q,s],
//   C_{s,q}[w,r] = wt_w G_sw[q,r], D_{s,p}[w,s] = G_sw[p,s]
#include <algorithm>
#include <type_traits>
#include "mfma_gemm.h"

namespace {

__device__ inline cplx bo_c(double v) { return cmake(v, 0.0); }
__device__ inline cplx bo_c(cplx v) { return v; }

constexpr int BO_BIG = 1 << 30;

// element (b, r, k) of a strided operand: b -> (b % bdiv, b / bdiv), k -> (k % kdiv, k / kdiv)
template <class T> struct Opd {
    const T *p = nullptr;
    long sb1 = 0, sb2 = 0, sr = 0, sk1 = 0, sk2 = 0;
    int bdiv = BO_BIG, kdiv = BO_BIG;
    __device__ cplx at(int b, int r, int k) const {
        return bo_c(p[(long)(b % bdiv) * sb1 + (long)(b / bdiv) * sb2 + (long)r * sr + (long)(k % kdiv) * sk1 +
                      (long)(k / kdiv) * sk2]);
    }
};

struct Dst {
    cplx *p = nullptr;
    long sb = 0, sr = 0, sc = 1;
    double alpha = 1.0;
    bool acc = false;
};

template <class TA, class TB> struct BoGemm {
    static constexpr bool A_CPLX = std::is_same<TA, cplx>::value, B_CPLX = std::is_same<TB, cplx>::value;
    int batch = 0, rows = 0, cols = 0, kdim = 0;
    Opd<TA> A;          // A.at(b, row, k)
    Opd<TB> B;          // B.at(b, col, k)
    Dst C;
    __device__ bool active(int) const { return true; }
    __device__ cplx loadA(int b, int row, int k) const { return A.at(b, row, k); }
    __device__ cplx loadB(int b, int k, int col) const { return B.at(b, col, k); }
    __device__ void store(int b, int row, int col, double re, double im) const {
        cplx *c = C.p + (long)b * C.sb + (long)row * C.sr + (long)col * C.sc;
        const cplx v = cmake(C.alpha * re, C.alpha * im);
        *c = C.acc ? cadd(*c, v) : v;
    }
};

template <class P> int bo_gemm(afq_handle *h, const P &p, const char *name) {
    if (p.batch <= 0 || p.rows <= 0 || p.cols <= 0) return AFQ_OK;
    afq_note_launch(h, name);
    hipError_t e = mfma_gemm_tasks(p.batch, p.rows, p.cols, 2, 2) >= 1024
                       ? launch_mfma_gemm<2, 2, P>(p, h->stream, 4)
                       : launch_mfma_gemm<1, 1, P>(p, h->stream, 4);
    if (e == hipSuccess) e = afq_post_launch(h);
    if (e != hipSuccess) { h->err = std::string("GEMM ") + name + ": " + hipGetErrorString(e); return AFQ_EHIP; }
    return AFQ_OK;
}

// the accumulation weight of afq_bp_update (bp_accumulate_kernel)
__global__ void bo_weights_kernel(const double *weight, const double *bp_cos, const cplx *bp_ph, int restore, int nw,
                                  cplx *wt) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    cplx v = cmake(weight[w], 0.0);
    if (restore == 1) v = cmul(v, bp_ph[w]);
    else if (restore == 2) v = cmul(v, cmake(bp_ph[w].x / bp_cos[w], bp_ph[w].y / bp_cos[w]));
    wt[w] = v;
}

// X[(w * 2 + s) * nL + x0 + j] = tr W[j * nw + w]
__global__ void bo_trace_kernel(const cplx *W, int N, int nw, int cur, int x0, int s, int nL, cplx *X) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= cur * nw) return;
    const int j = b / nw, w = b % nw;
    cplx t = cmake(0.0, 0.0);
    for (int n = 0; n < N; ++n) t = cadd(t, W[((long)b * N + n) * N + n]);
    X[((long)w * 2 + s) * nL + x0 + j] = t;
}

// the Coulomb-like terms on the diagonals: W1p_a += c_a, W1p_b += c_b, W1h_a += c_a
__global__ void bo_diag_kernel(cplx *W1pa, cplx *W1pb, cplx *W1ha, const cplx *X, int Na, int Nb, int nw, int cur,
                               int x0, int nL) {
    const int b = blockIdx.x, n = threadIdx.x;
    const int j = b / nw, w = b % nw;
    const cplx xa = X[((long)w * 2) * nL + x0 + j], xb = X[((long)w * 2 + 1) * nL + x0 + j];
    const cplx ca = cmake(-2.0 * xb.x - xa.x, -2.0 * xb.y - xa.y), cb = cmake(-xb.x, -xb.y);
    for (int i = n; i < Na; i += blockDim.x) {
        W1pa[((long)b * Na + i) * Na + i] = cadd(W1pa[((long)b * Na + i) * Na + i], ca);
        W1ha[((long)b * Na + i) * Na + i] = cadd(W1ha[((long)b * Na + i) * Na + i], ca);
    }
    for (int i = n; i < Nb; i += blockDim.x) W1pb[((long)b * Nb + i) * Nb + i] = cadd(W1pb[((long)b * Nb + i) * Nb + i], cb);
}

// S1h_b[w] += sum_j -X_b[w, x0 + j] R_b[j * nw + w]
__global__ void bo_s1hb_kernel(const cplx *R, const cplx *X, int Nb, int M, int nw, int cur, int x0, int nL, cplx *S) {
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long per = (long)Nb * M;
    if (e >= per * nw) return;
    const int w = (int)(e / per);
    const long r = e % per;
    cplx acc = S[e];
    for (int j = 0; j < cur; ++j) {
        const cplx xb = X[((long)w * 2 + 1) * nL + x0 + j];
        cfma(acc, cmake(-xb.x, -xb.y), R[((long)j * nw + w) * per + r]);
    }
    S[e] = acc;
}

__global__ void bo_scale_kernel(cplx *S, const cplx *wt, long per, int nw) {
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (e >= per * nw) return;
    S[e] = cmul(S[e], wt[e / per]);
}

// xbar[x] = sum_w wt_w (X_a + X_b)[w, x];  rbar = Gbar_a + Gbar_b
__global__ void bo_xbar_kernel(const cplx *X, const cplx *wt, int nw, int nL, cplx *xbar) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nL) return;
    cplx s = cmake(0.0, 0.0);
    for (int w = 0; w < nw; ++w) cfma(s, wt[w], cadd(X[((long)w * 2) * nL + x], X[((long)w * 2 + 1) * nL + x]));
    xbar[x] = s;
}

__global__ void bo_rbar_kernel(const cplx *Gbar, int M, cplx *rbar) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < M * M) rbar[e] = cadd(Gbar[e], Gbar[(long)M * M + e]);
}

// F1p[p,q] += 2 (sum_w wt_w) h1[p,q] + 2 sum_x xbar[x] L_x[q,p]
template <class LT>
__global__ void bo_lin_kernel(const LT *L, long ldL, long xsL, const cplx *xbar, int nL, const cplx *h1,
                              const cplx *wsum, int M, cplx *F) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= M * M) return;
    const int p = e / M, q = e % M;
    cplx c = cmake(0.0, 0.0);
    for (int x = 0; x < nL; ++x) cfma(c, xbar[x], bo_c(L[(long)x * xsL + (long)q * ldL + p]));
    const cplx t = cmul(*wsum, h1[e]);
    F[e] = cadd(F[e], cmake(2.0 * (t.x + c.x), 2.0 * (t.y + c.y)));
}

// walker-contiguous staging of the two-body RDM operands: [p, r, w]
__global__ void bo_stage_kernel(const cplx *G, const cplx *wt, int M, int nw, cplx *T0, cplx *T1, cplx *T2a,
                                cplx *T3a, cplx *T2b, cplx *T3b) {
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long mm = (long)M * M;
    if (e >= mm * nw) return;
    const long pr = e / nw;
    const int w = (int)(e % nw);
    const cplx ga = G[(long)w * 2 * mm + pr], gb = G[((long)w * 2 + 1) * mm + pr], s = cadd(ga, gb);
    const cplx a = wt[w], na = cmake(-a.x, -a.y);
    T0[e] = cmul(a, s); T1[e] = s;
    T2a[e] = cmul(na, ga); T3a[e] = ga;
    T2b[e] = cmul(na, gb); T3b[e] = gb;
}

struct Rdm2Prob {
    static constexpr bool A_CPLX = true, B_CPLX = true;
    int batch, rows, cols, kdim;          // M*M, M, M, 3 nw
    int M, nw;
    const cplx *T0, *T1, *T2a, *T3a, *T2b, *T3b;
    cplx *out;                            // [M, M, M, M], layout [p][r][q][s]
    __device__ bool active(int) const { return true; }
    __device__ cplx loadA(int b, int r, int k) const {
        const int seg = k / nw, w = k - seg * nw, p = b / M, q = b - p * M;
        if (seg == 0) return T0[((long)p * M + r) * nw + w];
        return (seg == 1 ? T2a : T2b)[((long)q * M + r) * nw + w];
    }
    __device__ cplx loadB(int b, int k, int s) const {
        const int seg = k / nw, w = k - seg * nw, p = b / M, q = b - p * M;
        if (seg == 0) return T1[((long)q * M + s) * nw + w];
        return (seg == 1 ? T3a : T3b)[((long)p * M + s) * nw + w];
    }
    __device__ void store(int b, int r, int s, double re, double im) const {
        const int p = b / M, q = b - p * M;
        out[(((long)p * M + r) * M + q) * M + s] = cmake(re, im);
    }
};

// workspace of the handle, grown on demand
cplx *bo_ws(afq_handle *h, size_t n, int *rc) {
    *rc = dev_grow(h, LT_WALKERS, &h->bpo_ws, &h->bpo_ws_len, n, "back-propagated observables");
    return h->bpo_ws;
}

#define BO_CK(call) do { if ((rc = (call))) return rc; } while (0)
#define BO_LAUNCH(...) do { AFQ_LAUNCH(h, __VA_ARGS__); AFQ_POST(h); } while (0)

template <class LT>
int bo_ekt(afq_handle *h, const LT *L, long ldL, long xsL, bool sym, const cplx *wt, cplx *F) {
    int rc = AFQ_OK;
    const int M = h->M, nw = h->nw, nt = h->nt, nL = h->bpo_nL;
    const int Ns[2] = {h->na, h->nb}, off[2] = {0, h->na};
    const int Na = h->na, Nb = h->nb;
    const long per = (long)M * nt;
    const cplx *Uc = h->phi_bp + per * nw;          // conj(phi_bp) [nw, M, nt]
    const cplx *V = h->ghalf;                       // [nw, nt, M]
    const cplx *Gbar = h->bp_est + 4, *wsum = h->bp_est + 3;
    // fixed part of the workspace
    const size_t nX = (size_t)nw * 2 * nL, nS = (size_t)nw * (Na + Nb) * M;
    const size_t fixed = nX + 2 * nS + (size_t)nL + (size_t)M * M;
    // per x: panels P, Q, R (both spins), T (alpha), W1p, W1h
    const size_t per_x = (size_t)nw * ((size_t)(sym ? 2 : 3) * (Na + Nb) * M + (sym ? 0 : (size_t)Na * M) +
                                       (size_t)Na * Na + (size_t)Nb * Nb + (size_t)Na * (Na + Nb));
    const size_t per_y = (size_t)M * M;
    // chunks of x: a fixed budget of 2^26 complex elements (1 GiB) of chunked scratch -- not derived from the free
    // memory, so that the chunking and the order of the sums are the same on every run -- or the afq_bp_ekt_chunks
    // lengths
    const size_t budget = (size_t)1 << 26;
    int nc = (int)std::max<size_t>(1, std::min<size_t>((size_t)nL, budget / std::max<size_t>(per_x, 1)));
    int ncy = (int)std::max<size_t>(1, std::min<size_t>((size_t)nL, budget / per_y));
    if (h->bpo_nc > 0) nc = std::min(h->bpo_nc, nL);
    if (h->bpo_ncy > 0) ncy = std::min(h->bpo_ncy, nL);
    cplx *ws = bo_ws(h, fixed + std::max((size_t)nc * per_x, (size_t)ncy * per_y), &rc);
    if (!ws) return rc;
    cplx *X = ws, *S1p = X + nX, *S1h = S1p + nS, *xbar = S1h + nS, *rbar = xbar + nL, *chunk = rbar + (size_t)M * M;
    cplx *S1p_s[2] = {S1p, S1p + (size_t)nw * Na * M}, *S1h_s[2] = {S1h, S1h + (size_t)nw * Na * M};
    AFQ_HIP(h, hipMemsetAsync(ws, 0, sizeof(cplx) * (nX + 2 * nS), h->stream));
    AFQ_HIP(h, hipMemsetAsync(F, 0, sizeof(cplx) * 2 * M * M, h->stream));

    for (int x0 = 0; x0 < nL; x0 += nc) {
        const int cur = std::min(nc, nL - x0);
        const int nb = cur * nw;
        cplx *P[2], *Q[2], *R[2], *T, *W1p[2], *W1h[2];
        cplx *c = chunk;
        for (int s = 0; s < 2; ++s) { P[s] = c; c += (size_t)nb * Ns[s] * M; }
        for (int s = 0; s < 2; ++s) { R[s] = c; c += (size_t)nb * Ns[s] * M; }
        if (sym) { Q[0] = P[0]; Q[1] = P[1]; T = R[0]; }
        else {
            for (int s = 0; s < 2; ++s) { Q[s] = c; c += (size_t)nb * Ns[s] * M; }
            T = c; c += (size_t)nb * Na * M;
        }
        for (int s = 0; s < 2; ++s) { W1p[s] = c; c += (size_t)nb * Ns[s] * Ns[s]; }
        for (int s = 0; s < 2; ++s) { W1h[s] = c; c += (size_t)nb * Na * Ns[s]; }

        for (int s = 0; s < 2; ++s) {
            const int N = Ns[s];
            if (!N) continue;
            // P = U^T L_x, Q = U^T L_x^T           (batch b = j nw + w)
            BoGemm<cplx, LT> g;
            g.batch = nb; g.rows = N; g.cols = M; g.kdim = M;
            g.A.p = Uc + off[s]; g.A.bdiv = nw; g.A.sb1 = per; g.A.sr = 1; g.A.sk1 = nt;
            g.B.p = L + (long)x0 * xsL; g.B.bdiv = nw; g.B.sb2 = xsL; g.B.sr = 1; g.B.sk1 = ldL;
            g.C.p = P[s]; g.C.sb = (long)N * M; g.C.sr = M;
            BO_CK(bo_gemm(h, g, "bp_obs panel U^T L"));
            if (!sym) {
                g.B.sr = ldL; g.B.sk1 = 1; g.C.p = Q[s];
                BO_CK(bo_gemm(h, g, "bp_obs panel U^T L^T"));
            }
            // R = V L_x, T = V_a L_x^T
            BoGemm<cplx, LT> r = g;
            r.A.p = V + (long)off[s] * M; r.A.sb1 = (long)nt * M; r.A.sr = M; r.A.sk1 = 1;
            r.B.sr = 1; r.B.sk1 = ldL; r.C.p = R[s];
            BO_CK(bo_gemm(h, r, "bp_obs panel V L"));
            if (!sym && s == 0) {
                r.B.sr = ldL; r.B.sk1 = 1; r.C.p = T;
                BO_CK(bo_gemm(h, r, "bp_obs panel V L^T"));
            }
            // W1p = P V^T and its trace X_s[x]
            BoGemm<cplx, cplx> w;
            w.batch = nb; w.rows = N; w.cols = N; w.kdim = M;
            w.A.p = P[s]; w.A.sb1 = (long)N * M; w.A.sr = M; w.A.sk1 = 1;
            w.B.p = V + (long)off[s] * M; w.B.bdiv = nw; w.B.sb1 = (long)nt * M; w.B.sr = M; w.B.sk1 = 1;
            w.C.p = W1p[s]; w.C.sb = (long)N * N; w.C.sr = N;
            BO_CK(bo_gemm(h, w, "bp_obs W = P V^T"));
            BO_LAUNCH(bo_trace_kernel, dim3((nb + 127) / 128), dim3(128), 0, h->stream, W1p[s], N, nw, cur, x0, s, nL, X);
        }
        if (Na) {
            // W1h(s) = T U_s
            for (int s = 0; s < 2; ++s) {
                if (!Ns[s]) continue;
                BoGemm<cplx, cplx> w;
                w.batch = nb; w.rows = Na; w.cols = Ns[s]; w.kdim = M;
                w.A.p = T; w.A.sb1 = (long)Na * M; w.A.sr = M; w.A.sk1 = 1;
                w.B.p = Uc + off[s]; w.B.bdiv = nw; w.B.sb1 = per; w.B.sr = 1; w.B.sk1 = nt;
                w.C.p = W1h[s]; w.C.sb = (long)Na * Ns[s]; w.C.sr = Ns[s];
                BO_CK(bo_gemm(h, w, "bp_obs W' = T U"));
            }
        }
        BO_LAUNCH(bo_diag_kernel, dim3(nb), dim3(64), 0, h->stream, W1p[0], W1p[1], W1h[0], X, Na, Nb, nw, cur, x0, nL);
        // S1p_s[w] += sum_(j, m) W1p_s[j nw + w][n, m] Q_s[j nw + w][m, k]
        for (int s = 0; s < 2; ++s) {
            const int N = Ns[s];
            if (!N) continue;
            BoGemm<cplx, cplx> g;
            g.batch = nw; g.rows = N; g.cols = M; g.kdim = cur * N;
            g.A.p = W1p[s]; g.A.sb1 = (long)N * N; g.A.sr = N; g.A.sk1 = 1; g.A.kdiv = N; g.A.sk2 = (long)nw * N * N;
            g.B.p = Q[s]; g.B.sb1 = (long)N * M; g.B.sr = 1; g.B.sk1 = M; g.B.kdiv = N; g.B.sk2 = (long)nw * N * M;
            g.C.p = S1p_s[s]; g.C.sb = (long)N * M; g.C.sr = M; g.C.acc = true;
            BO_CK(bo_gemm(h, g, "bp_obs S1p += W Q"));
        }
        // S1h_a[w] += sum_(j, m) W1h_s[j nw + w][n, m] R_s[j nw + w][m, k]; S1h_b[w] -= sum_j X_b R_b
        for (int s = 0; s < 2 && Na; ++s) {
            const int N = Ns[s];
            if (!N) continue;
            BoGemm<cplx, cplx> g;
            g.batch = nw; g.rows = Na; g.cols = M; g.kdim = cur * N;
            g.A.p = W1h[s]; g.A.sb1 = (long)Na * N; g.A.sr = N; g.A.sk1 = 1; g.A.kdiv = N; g.A.sk2 = (long)nw * Na * N;
            g.B.p = R[s]; g.B.sb1 = (long)N * M; g.B.sr = 1; g.B.sk1 = M; g.B.kdiv = N; g.B.sk2 = (long)nw * N * M;
            g.C.p = S1h_s[0]; g.C.sb = (long)Na * M; g.C.sr = M; g.C.acc = true;
            BO_CK(bo_gemm(h, g, "bp_obs S1h += W' R"));
        }
        if (Nb) {
            const long n = (long)nw * Nb * M;
            BO_LAUNCH(bo_s1hb_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, R[1], X, Nb, M, nw, cur,
                      x0, nL, S1h_s[1]);
        }
    }
    // closing products over (w, n), weighted
    for (int s = 0; s < 2; ++s) {
        const long n = (long)nw * Ns[s] * M;
        if (!n) continue;
        BO_LAUNCH(bo_scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, S1p_s[s], wt, n / nw, nw);
        BO_LAUNCH(bo_scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, S1h_s[s], wt, n / nw, nw);
    }
    for (int s = 0; s < 2; ++s) {
        const int N = Ns[s];
        if (!N) continue;
        BoGemm<cplx, cplx> g;                       // F1p += sum_(w, n) V_s[w][n, p] S1p_s[w][n, q]
        g.batch = 1; g.rows = M; g.cols = M; g.kdim = nw * N;
        g.A.p = V + (long)off[s] * M; g.A.sr = 1; g.A.sk1 = M; g.A.kdiv = N; g.A.sk2 = (long)nt * M;
        g.B.p = S1p_s[s]; g.B.sr = 1; g.B.sk1 = M;
        g.C.p = F; g.C.sr = M; g.C.acc = true;
        BO_CK(bo_gemm(h, g, "bp_obs F1p += V^T S"));
        g.A.p = Uc + off[s]; g.A.sr = nt; g.A.sk1 = 1; g.A.kdiv = N; g.A.sk2 = per;   // F1h += sum U_s[w][p, n] S1h_s[w][n, q]
        g.B.p = S1h_s[s];
        g.C.p = F + (long)M * M;
        BO_CK(bo_gemm(h, g, "bp_obs F1h += U S"));
    }
    // terms linear in G, on Gbar
    BO_LAUNCH(bo_xbar_kernel, dim3((nL + 127) / 128), dim3(128), 0, h->stream, X, wt, nw, nL, xbar);
    BO_LAUNCH(bo_rbar_kernel, dim3((M * M + 255) / 256), dim3(256), 0, h->stream, Gbar, M, rbar);
    BO_LAUNCH(bo_lin_kernel<LT>, dim3((M * M + 127) / 128), dim3(128), 0, h->stream, L, ldL, xsL, xbar, nL, h->bpo_h1,
              wsum, M, F);
    {
        BoGemm<cplx, cplx> g;                       // F1p -= rbar^T h1
        g.batch = 1; g.rows = M; g.cols = M; g.kdim = M;
        g.A.p = rbar; g.A.sr = 1; g.A.sk1 = M;
        g.B.p = h->bpo_h1; g.B.sr = 1; g.B.sk1 = M;
        g.C.p = F; g.C.sr = M; g.C.acc = true; g.C.alpha = -1.0;
        BO_CK(bo_gemm(h, g, "bp_obs F1p -= Gbar^T h1"));
        g.A.sr = M; g.A.sk1 = 1;                    // F1h -= rbar h1^T
        g.B.sr = M; g.B.sk1 = 1;
        g.C.p = F + (long)M * M;
        BO_CK(bo_gemm(h, g, "bp_obs F1h -= Gbar h1^T"));
    }
    for (int x0 = 0; x0 < nL; x0 += ncy) {          // F1p -= sum_x L_x rbar^T L_x^T
        const int cur = std::min(ncy, nL - x0);
        cplx *Y = chunk;
        BoGemm<LT, cplx> y;                         // Y_x = L_x rbar^T
        y.batch = cur; y.rows = M; y.cols = M; y.kdim = M;
        y.A.p = L + (long)x0 * xsL; y.A.sb1 = xsL; y.A.sr = ldL; y.A.sk1 = 1;
        y.B.p = rbar; y.B.sr = M; y.B.sk1 = 1;
        y.C.p = Y; y.C.sb = (long)M * M; y.C.sr = M;
        BO_CK(bo_gemm(h, y, "bp_obs Y = L Gbar^T"));
        BoGemm<cplx, LT> g;                         // F1p -= sum_(j, k) Y_j[i, k] L_j[l, k]
        g.batch = 1; g.rows = M; g.cols = M; g.kdim = cur * M;
        g.A.p = Y; g.A.sr = M; g.A.sk1 = 1; g.A.kdiv = M; g.A.sk2 = (long)M * M;
        g.B.p = L + (long)x0 * xsL; g.B.sr = ldL; g.B.sk1 = 1; g.B.kdiv = M; g.B.sk2 = xsL;
        g.C.p = F; g.C.sr = M; g.C.acc = true; g.C.alpha = -1.0;
        BO_CK(bo_gemm(h, g, "bp_obs F1p -= Y L^T"));
    }
    return AFQ_OK;
}

int bo_two_rdm(afq_handle *h, const cplx *wt, cplx *out) {
    int rc = AFQ_OK;
    const int M = h->M, nw = h->nw;
    const size_t n = (size_t)M * M * nw;
    cplx *ws = bo_ws(h, 6 * n, &rc);
    if (!ws) return rc;
    BO_LAUNCH(bo_stage_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->G, wt, M, nw, ws, ws + n,
              ws + 2 * n, ws + 3 * n, ws + 4 * n, ws + 5 * n);
    Rdm2Prob p;
    p.batch = M * M; p.rows = M; p.cols = M; p.kdim = 3 * nw; p.M = M; p.nw = nw;
    p.T0 = ws; p.T1 = ws + n; p.T2a = ws + 2 * n; p.T3a = ws + 3 * n; p.T2b = ws + 4 * n; p.T3b = ws + 5 * n;
    p.out = out;
    return bo_gemm(h, p, "bp_obs two-body RDM");
}

}  // namespace

int k_bp_observables(afq_handle *h, int restore, cplx *two_out, cplx *fock_out) {
    int rc = AFQ_OK;
    BO_CK(dev_ensure(h, LT_WALKERS, &h->bpo_wt, (size_t)h->nw));
    BO_LAUNCH(bo_weights_kernel, dim3((h->nw + 127) / 128), dim3(128), 0, h->stream, h->weight, h->bp_cos, h->bp_ph,
              restore, h->nw, h->bpo_wt);
    if (two_out) BO_CK(bo_two_rdm(h, h->bpo_wt, two_out));
    if (fock_out) {
        const int M = h->M, Mp = (M + 1) & ~1;
        if (h->bpo_L) BO_CK(bo_ekt<cplx>(h, h->bpo_L, M, (long)M * M, false, h->bpo_wt, fock_out));
        else {
            BO_CK(k_fullg_expand(h));
            BO_CK(bo_ekt<double>(h, h->L_full, Mp, (long)M * Mp, h->hs_sym, h->bpo_wt, fock_out));
        }
    }
    return AFQ_OK;
}
