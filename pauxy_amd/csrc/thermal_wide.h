// The stratified Green's function of a thermal walker beyond one lane per column (T = cplx: AFQ_THERMAL_WIDE, the
// continuous fields; T = double: AFQ_THERMAL_DELAYED, the discrete fields, thermal_greens_wide_kernel in the trace): the
// algorithm of thermal_strat.h -- column-pivoted Householder QR of the first bin, norms recomputed every step, ties to
// the lower index; C = (B Q) D, Q D t = C, T <- t T for every further bin; D split at |D| = 1; one pivoted solve of
// (D_b Q^H + D_s T) G = D_b Q^H; det G by LU with partial pivoting -- with ONE M x (M | 1) matrix of T in LDS and a
// lane that owns two columns (c and c + 64), so M <= 128 lanes-wise; the 160 KiB of a compute unit hold a complex matrix
// to M = 95 and a real one beyond the lanes (141,824 B at M = 128).
//
// Everything but the one matrix lives in the work-group's own scratch in device memory, four [M, M] buffers (pitch M):
//   Ta, Tb   T, used in turn by T <- t T (ts_gemm with both operands read from scratch by its loaders);
//   Pn       the reflectors of the last QR, transposed (reflector j contiguous at Pn + j M, v_0 = 1 implied); at the
//            end the LU factors of the solve, transposed as well (column k contiguous);
//   Xs       t = D^-1 R P^T of the bins behind the first; at the end the right-hand side D_b Q^H.
// A work-group reads back only what it has written itself, across a __syncthreads(): the discipline of every user of
// the handle's th_scratch.
//
// Q is never accumulated.  The QR leaves reflector j below the diagonal of column j of W and tau_j in LDS; behind the QR
// t and the reflectors go to scratch, the next bin B is loaded into the same LDS matrix, H_0 .. H_(M-1) are applied to
// it from the right and its columns scaled by D: (B Q) D in place with O(M^2) device traffic per bin.  For the closing
// solve Q^H = H_(M-1) .. H_0 is built in LDS from the identity.  The solve cannot hold X and the right-hand side side
// by side as ts_solve does: X is factored in LDS (LU, partial pivoting, multipliers kept), the factors go to scratch, the
// right-hand side comes into LDS through the row permutation and is substituted forward and back, column k of the
// factors read from scratch at step k.  The results are those of the resident and the streamed engine to rounding, not
// to the bit (B Q by reflectors, not by a product with an accumulated Q; LU and substitution, not Gauss-Jordan).
//
// The invariants of the other engines hold: no loop whose trip count depends on data, exits that are uniform over the
// work-group (a zero pivot of det G, seen by every thread alike), every wave at every barrier; the same bits on repeat
// and at any grid position.
//
// The engine enters thermal_strat.h's one kernel and one launcher as TsWide<T>.  Behind it, what needs every engine in
// sight: th_launch_greens<T>, which picks the engine by the handle's th_engine, and th_screen_bound, the one refusal of
// an M that a route's kernels or lanes do not hold.
//
// TsFar<T> (AFQ_THERMAL_FAR, the complex walkers) is the same body with the one matrix out of LDS as well: W is a fifth
// buffer of the work-group's scratch, M x (M | 1) behind the four [M, M], and LDS holds the vectors alone (18,944 B for
// cplx).  Where W lives is the body's one template parameter; every helper takes W as a pointer and every element goes
// through the same operations in the same order, so the two placements give the same bits where both run.  The lanes
// bind: M <= 128, which holds the shell of 123 plane waves and the lattices 10 x 10, 11 x 11 and 8 x 16.
//
// TsQuad<cplx> (AFQ_THERMAL_QUAD) is the far placement with four columns per lane.  The columns a lane owns are the
// body's third template parameter NC (2: TsWide, TsFar; 4: TsQuad), and every vector of the body -- D, v, part, aux with
// tau and the second reflector buffer in it, perm, the colv / rowr of the LU and the substitution -- is sized and
// addressed by COLS = 64 NC.  A column meets the same operations in the same order whatever NC is, so the quad engine
// gives the far engine's bits to M = 128, and reaches M <= 256: the shells to 251 plane waves and the lattices 12 x 12
// and 16 x 16.  LDS: 37,888 B.  The invariants above hold for it unchanged.
#pragma once
#include "thermal_strat.h"
#include <initializer_list>
#include <string>

#define TW_COLS 128             // two columns per lane
#define TQ_COLS 256             // four columns per lane (TsQuad)

namespace {

// LDS of the wide Green's kernel: one matrix; D[128], v[128], part[512], aux[384] scalars; perm[128]
template <class T> inline size_t ts_greens_wide_lds(int M) { return sizeof(T) * (ts_mat(M) + 128 + 128 + 512 + 384) + sizeof(int) * TW_COLS; }
// scalars of device scratch per work-group
__host__ __device__ inline size_t ts_greens_wide_scratch(int M) { return 4 * (size_t)M * M; }
// LDS of the far Green's kernel: the same vectors and no matrix
template <class T> inline size_t ts_greens_far_lds(int) { return sizeof(T) * (128 + 128 + 512 + 384) + sizeof(int) * TW_COLS; }
// its scratch: the four [M, M] buffers and W [M, M | 1] behind them
__host__ __device__ inline size_t ts_greens_far_scratch(int M) { return 4 * (size_t)M * M + ts_mat(M); }
// LDS of the quad Green's kernel: the far kernel's vectors at 256 columns -- D[256], v[256], part[1024], aux[768]; perm[256]
template <class T> inline size_t ts_greens_quad_lds(int) { return sizeof(T) * (TQ_COLS + TQ_COLS + 4 * TQ_COLS + 3 * TQ_COLS) + sizeof(int) * TQ_COLS; }

// NC, here and below: the columns a lane owns (2 or 4); COLS = 64 NC is the pitch of every vector of the body
template <int NC, class T> __device__ inline T tw_sum4(const T *p) {
    typedef TsScalar<T> S;
    constexpr int COLS = 64 * NC;
    return S::add(S::add(p[0], p[COLS]), S::add(p[2 * COLS], p[3 * COLS]));
}

// W[j.., cc] <- (I - tau v v^H) W[j.., cc] for the columns cmin <= cc < M, NC per lane and four row classes per column;
// v[j .. M - 1] in LDS, written behind a barrier.  One barrier inside; none behind the update.  part: 4 COLS scalars.
template <int NC, class T> __device__ inline void tw_reflect_left(T *W, int M, int LD, int j, int cmin, const T *v, double tau, T *part) {
    constexpr int COLS = 64 * NC;
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
#pragma unroll
    for (int h = 0; h < NC; ++h) {
        const int cc = c + 64 * h;
        if (cc >= cmin && cc < M) {
            T s = TsScalar<T>::zero();
            for (int i = j + q; i < M; i += 4) TsScalar<T>::fma(s, TsScalar<T>::conj(v[i]), W[i * LD + cc]);
            part[q * COLS + cc] = s;
        }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < NC; ++h) {
        const int cc = c + 64 * h;
        if (cc >= cmin && cc < M) {
            const T s = TsScalar<T>::scale(tw_sum4<NC, T>(part + cc), -tau);
            for (int i = j + q; i < M; i += 4) TsScalar<T>::fma(W[i * LD + cc], s, v[i]);
        }
    }
}

// Column-pivoted Householder QR of W [M, M] (LDS, pitch LD), in place: W P = Q R.  On return the upper triangle of W
// holds R, column j below the diagonal reflector j (v_0 = 1 implied), tau[j] its factor, perm[j] the original column now
// at position j.  The pivot of step j: the remaining column of the largest norm over the rows j.., recomputed every
// step, ties to the lower index; every wave runs the search on its own over the NC columns of its lanes.
template <int NC, class T> __device__ void tw_qrcp(T *W, int M, int LD, int *perm, T *v, T *part, double *tau) {
    typedef TsScalar<T> S;
    constexpr int COLS = 64 * NC;
    const int tid = threadIdx.x, c = tid & 63, q = tid >> 6;
    if (tid < M) perm[tid] = tid;
    __syncthreads();
    for (int j = 0; j < M; ++j) {
#pragma unroll
        for (int h = 0; h < NC; ++h) {
            const int cc = c + 64 * h;
            if (cc >= j && cc < M) {
                double s = 0.0;
                for (int i = j + q; i < M; i += 4) S::abs2(s, W[i * LD + cc]);
                S::re(part[q * COLS + cc]) = s;
            }
        }
        __syncthreads();
        double nrm2 = -1.0;
        int piv = j;
#pragma unroll
        for (int h = 0; h < NC; ++h) {                                // (low column first: a tie stays with it)
            const int cc = c + 64 * h;
            if (cc >= j && cc < M) {
                const double n = (S::re(part[cc]) + S::re(part[COLS + cc])) + (S::re(part[2 * COLS + cc]) + S::re(part[3 * COLS + cc]));
                if (n > nrm2) { nrm2 = n; piv = cc; }
            }
        }
        ts_wave_argmax(nrm2, piv);
        if (piv != j) {
            if (tid < M) { const T t = W[tid * LD + j]; W[tid * LD + j] = W[tid * LD + piv]; W[tid * LD + piv] = t; }
            if (tid == TH_THREADS - 1) { const int t = perm[j]; perm[j] = perm[piv]; perm[piv] = t; }
        }
        __syncthreads();
        const T x0 = W[j * LD + j];
        const double nrm = sqrt(nrm2), ax0 = S::abs(x0);
        const T ph = ax0 > 0.0 ? S::unit(x0, ax0) : S::real(1.0);
        const T alpha = S::scale(S::neg(ph), nrm);                  // H x = alpha e_0, |x_0 - alpha| = |x_0| + ||x||
        const double tj = nrm > 0.0 ? (nrm + ax0) / nrm : 0.0;
        const T den = S::scale(ph, ax0 + nrm);                      // x_0 - alpha, no cancellation
        if (tid < M - j)
            v[j + tid] = (tid == 0 || !(nrm > 0.0)) ? S::real(tid == 0 ? 1.0 : 0.0) : S::div(W[(j + tid) * LD + j], den);
        if (tid == 0) tau[j] = tj;
        __syncthreads();
        tw_reflect_left<NC>(W, M, LD, j, j + 1, v, tj, part);
        // column j: R's diagonal, and the reflector where the zeros would be
        if (c == (j & 63) && nrm > 0.0) for (int i = j + q; i < M; i += 4) W[i * LD + j] = i == j ? alpha : v[i];
        __syncthreads();
    }
}

// Behind tw_qrcp: t = D^-1 R P^T into tdst [M, M] (device), the reflectors transposed into Pn, D = diag R.
template <class T> __device__ inline void tw_store_qr(const T *W, int M, int LD, const int *perm, T *tdst, T *Pn, T *D) {
    typedef TsScalar<T> S;
    const int tid = threadIdx.x;
    for (int e = tid; e < M * M; e += TH_THREADS) {
        const int i = e / M, j = e % M;
        const T w = W[i * LD + j];
        tdst[i * M + perm[j]] = j >= i ? S::div(w, W[i * LD + i]) : S::zero();
        if (i > j) Pn[j * M + i] = w;
    }
    if (tid < M) D[tid] = W[tid * LD + tid];
    __syncthreads();
}

// reflector j out of Pn into v[j .. M - 1]
template <class T> __device__ inline void tw_load_reflector(T *v, const T *Pn, int M, int j) {
    const int tid = threadIdx.x;
    if (tid < M - j) v[j + tid] = tid == 0 ? TsScalar<T>::real(1.0) : Pn[j * M + j + tid];
}

// W <- W H_0 H_1 .. H_(M-1) = W Q: row r of W by the two threads r and r + 128 (the k of even and of odd distance from
// j; with four columns per lane the pair takes row r + 128 as well), then every element of the trailing columns by the
// whole work-group.  v0, v1: COLS scalars each, used in turn.
template <int NC, class T> __device__ void tw_apply_right(T *W, int M, int LD, const T *Pn, const double *tau, T *v0, T *v1, T *part) {
    typedef TsScalar<T> S;
    constexpr int COLS = 64 * NC;
    const int tid = threadIdx.x, r = tid & 127, hh = tid >> 7;
    for (int j = 0; j < M; ++j) {
        T *v = (j & 1) ? v1 : v0;
        tw_load_reflector(v, Pn, M, j);
        __syncthreads();
#pragma unroll
        for (int g = 0; g < NC / 2; ++g) {
            const int rw = r + 128 * g;
            if (rw < M) {
                T s = S::zero();
                for (int i = j + hh; i < M; i += 2) S::fma(s, W[rw * LD + i], v[i]);
                part[hh * COLS + rw] = s;
            }
        }
        __syncthreads();
        const double tj = tau[j];
        const int n = M - j;
        for (int e = tid; e < M * n; e += TH_THREADS) {
            const int rr = e / n, i = j + e % n;
            const T s = S::scale(S::add(part[rr], part[COLS + rr]), -tj);
            S::fma(W[rr * LD + i], s, S::conj(v[i]));
        }
    }
    __syncthreads();
}

// W <- Q^H = H_(M-1) .. H_0 I
template <int NC, class T> __device__ void tw_build_qt(T *W, int M, int LD, const T *Pn, const double *tau, T *v0, T *v1, T *part) {
    const int tid = threadIdx.x;
    for (int e = tid; e < M * M; e += TH_THREADS) { const int r = e / M, c = e % M; W[r * LD + c] = TsScalar<T>::real(r == c ? 1.0 : 0.0); }
    for (int j = 0; j < M; ++j) {
        T *v = (j & 1) ? v1 : v0;
        tw_load_reflector(v, Pn, M, j);
        __syncthreads();
        tw_reflect_left<NC>(W, M, LD, j, 0, v, tau[j], part);
    }
    __syncthreads();
}

// LU of X [M, M] (LDS) with partial (row) pivoting, in place: the multipliers below the diagonal, rows exchanged whole,
// rperm[i] the original row now at i.  Returns the product of the pivots with the sign of the exchanges (the same value
// in every thread).  DET: a zero pivot ends the factorisation with 0 (uniform over the work-group).  colv: COLS scalars;
// a lane searches its NC rows from the low one up.
template <int NC, bool DET, class T> __device__ T tw_lu(T *X, int M, int LD, int *rperm, T *colv) {
    typedef TsScalar<T> S;
    const int tid = threadIdx.x, c = tid & 63;
    T det = S::real(1.0);
    if (tid < M) rperm[tid] = tid;
    for (int k = 0; k < M; ++k) {
        double a = -1.0;
        int p = k;
#pragma unroll
        for (int h = 0; h < NC; ++h) {
            const int rr = c + 64 * h;
            if (rr >= k && rr < M) {
                const double ar = S::abs(X[rr * LD + k]);
                if (ar > a) { a = ar; p = rr; }
            }
        }
        ts_wave_argmax(a, p);
        __syncthreads();                                  // (every wave has read column k before rows move)
        if (p != k) {
            if (tid < M) { const T t = X[k * LD + tid]; X[k * LD + tid] = X[p * LD + tid]; X[p * LD + tid] = t; }
            if (tid == TH_THREADS - 1) { const int t = rperm[k]; rperm[k] = rperm[p]; rperm[p] = t; }
            det = S::neg(det);
        }
        __syncthreads();
        const T piv = X[k * LD + k];                      // (the same value in every thread: uniform branches below)
        det = S::mul(det, piv);
        if (DET && S::is_zero(piv)) return S::zero();
        if (tid > k && tid < M) { const T m = S::div(X[tid * LD + k], piv); colv[tid] = m; X[tid * LD + k] = m; }
        __syncthreads();
        const int n = M - k - 1;
        for (int e = tid; e < n * n; e += TH_THREADS) {
            const int i = k + 1 + e / n, cc = k + 1 + e % n;
            S::fma(X[i * LD + cc], S::neg(colv[i]), X[k * LD + cc]);
        }
        __syncthreads();
    }
    return det;
}

// L U G = R' with the factors transposed in LUt (device: column k at LUt + k M) and R' [M, M] in LDS, which G
// overwrites.  c0, c1: M <= COLS scalars each, used in turn; rowr: as many (no lane owns a column here: nothing to widen).
template <class T> __device__ void tw_substitute(T *R, int M, int LD, const T *LUt, T *c0, T *c1, T *rowr) {
    typedef TsScalar<T> S;
    const int tid = threadIdx.x;
    for (int k = 0; k < M - 1; ++k) {                     // L y = R', unit diagonal
        T *cv = (k & 1) ? c1 : c0;
        if (tid > k && tid < M) cv[tid] = LUt[k * M + tid];
        __syncthreads();
        const int n = M - k - 1;
        for (int e = tid; e < n * M; e += TH_THREADS) {
            const int i = k + 1 + e / M, cc = e % M;
            S::fma(R[i * LD + cc], S::neg(cv[i]), R[k * LD + cc]);
        }
    }
    __syncthreads();
    for (int k = M - 1; k >= 0; --k) {                    // U G = y
        if (tid < k) c0[tid] = LUt[k * M + tid];
        if (tid < M) {
            const T x = S::div(R[k * LD + tid], LUt[k * M + k]);
            rowr[tid] = x;
            R[k * LD + tid] = x;
        }
        __syncthreads();
        for (int e = tid; e < k * M; e += TH_THREADS) {
            const int i = e / M, cc = e % M;
            S::fma(R[i * LD + cc], S::neg(c0[i]), rowr[cc]);
        }
        __syncthreads();
    }
}

// The work of one work-group, as ts_greens_body (another algorithm: its own body); scr: the work-group's own
// ts_greens_wide_scratch(M) scalars, or with FAR ts_greens_far_scratch(M): W then lies behind the four buffers in
// device memory and the vectors start at smem.
template <class T, bool FAR, int NC>
__device__ __forceinline__ void ts_greens_wide_body(unsigned char *smem, const T *Bw, T *scr, int M, int nbins, int first,
                                                    T *Gd, T *Gd2, T *detd) {
    typedef TsScalar<T> S;
    constexpr int COLS = 64 * NC;                                    // 128 or 256: what every vector below holds
    const int LD = M | 1, tid = threadIdx.x;
    const size_t mat = ts_mat(M);
    const long mm = (long)M * M;
    T *W = FAR ? scr + 4 * mm : (T *)smem;
    T *D = FAR ? (T *)smem : W + mat, *v = D + COLS, *part = v + COLS, *aux = part + 4 * COLS;
    int *perm = (int *)(aux + 3 * COLS);
    double *tau = (double *)aux;                                     // COLS doubles: the first half of as many cplx, all of as many double
    T *v1 = aux + COLS * sizeof(double) / sizeof(T);                 // the second reflector buffer: the COLS scalars behind tau
    T *Tin = scr, *Tout = scr + mm, *Pn = scr + 2 * mm, *Xs = scr + 3 * mm;

    {
        const T *B = Bw + (long)first * 2 * mm;
        for (int e = tid; e < M * M; e += TH_THREADS) W[(e / M) * LD + e % M] = B[e];
    }
    __syncthreads();
    tw_qrcp<NC>(W, M, LD, perm, v, part, tau);
    tw_store_qr(W, M, LD, perm, Tin, Pn, D);                         // T = D^-1 R P^T
    for (int n = 1; n < nbins; ++n) {
        const T *B = Bw + (long)((first + n) % nbins) * 2 * mm;
        for (int e = tid; e < M * M; e += TH_THREADS) W[(e / M) * LD + e % M] = B[e];
        __syncthreads();
        tw_apply_right<NC>(W, M, LD, Pn, tau, v, v1, part);              // B Q
        for (int e = tid; e < M * M; e += TH_THREADS) {
            const int r = e / M, c = e % M;
            W[r * LD + c] = S::mul(W[r * LD + c], D[c]);             // (B Q) D
        }
        __syncthreads();
        tw_qrcp<NC>(W, M, LD, perm, v, part, tau);
        tw_store_qr(W, M, LD, perm, Xs, Pn, D);
        // T <- t T
        ts_gemm<T>(M, [&](int r, int k) { return Xs[r * M + k]; }, [&](int k, int c) { return Tin[k * M + c]; },
                   [&](int r, int c, T x) { Tout[r * M + c] = x; });
        __syncthreads();
        T *t = Tin; Tin = Tout; Tout = t;
    }
    // (D_b Q^H + D_s T) G = D_b Q^H, D_b = 1 / |D| and D_s = D / |D| where |D| > 1, else D_b = 1 and D_s = D
    tw_build_qt<NC>(W, M, LD, Pn, tau, v, v1, part);
    for (int e = tid; e < M * M; e += TH_THREADS) {
        const int i = e / M, j = e % M;
        const T d = D[i];
        const double ad = S::abs(d);
        const double db = ad > 1.0 ? 1.0 / ad : 1.0;
        const T ds = ad > 1.0 ? S::unit(d, ad) : d;
        const T r = S::scale(W[i * LD + j], db);
        T x = r;
        S::fma(x, ds, Tin[i * M + j]);
        W[i * LD + j] = x;
        Xs[i * M + j] = r;
    }
    __syncthreads();
    tw_lu<NC, false>(W, M, LD, perm, aux);
    for (int e = tid; e < M * M; e += TH_THREADS) { const int r = e / M, c = e % M; Pn[c * M + r] = W[r * LD + c]; }
    __syncthreads();
    for (int e = tid; e < M * M; e += TH_THREADS) { const int r = e / M, c = e % M; W[r * LD + c] = Xs[perm[r] * M + c]; }
    __syncthreads();
    tw_substitute(W, M, LD, Pn, aux, aux + COLS, aux + 2 * COLS);
    for (int e = tid; e < M * M; e += TH_THREADS) {
        const T g = W[(e / M) * LD + e % M];
        Gd[e] = g;
        if (Gd2) Gd2[e] = g;
    }
    if (!detd) return;
    __syncthreads();
    const T dg = tw_lu<NC, true>(W, M, LD, perm, aux);
    if (tid == 0) *detd = dg;
}

// The wide engine of thermal_greens_kernel (thermal_strat.h): scratch [work-groups, 4, M, M].  Its own names in the
// trace.  The sweep is the one kernel's: every work-group of the grid (2 nw, bins) works in a scratch of its own.
template <class T> struct TsWide {
    static constexpr bool has_sweep = true;
    static size_t lds(int M) { return ts_greens_wide_lds<T>(M); }
    __host__ __device__ static size_t scratch(int M) { return ts_greens_wide_scratch(M); }
    static const char *name(bool sweep) {
        return std::is_same<T, cplx>::value ? (sweep ? "thermal_cgreens_wide_sweep_kernel" : "thermal_cgreens_wide_kernel")
                                            : (sweep ? "thermal_greens_wide_sweep_kernel" : "thermal_greens_wide_kernel");
    }
    __device__ __forceinline__ static void body(unsigned char *smem, const T *Bw, T *scr, int M, int nbins, int first, T *Gd, T *Gd2, T *detd) {
        ts_greens_wide_body<T, false, 2>(smem, Bw, scr, M, nbins, first, Gd, Gd2, detd);
    }
};

// The far engine: the wide body with W in the work-group's scratch as well, [work-groups, 4 M M + M (M | 1)].
template <class T> struct TsFar {
    static constexpr bool has_sweep = true;
    static size_t lds(int M) { return ts_greens_far_lds<T>(M); }
    __host__ __device__ static size_t scratch(int M) { return ts_greens_far_scratch(M); }
    static const char *name(bool sweep) {
        return std::is_same<T, cplx>::value ? (sweep ? "thermal_cgreens_far_sweep_kernel" : "thermal_cgreens_far_kernel")
                                            : (sweep ? "thermal_greens_far_sweep_kernel" : "thermal_greens_far_kernel");
    }
    __device__ __forceinline__ static void body(unsigned char *smem, const T *Bw, T *scr, int M, int nbins, int first, T *Gd, T *Gd2, T *detd) {
        ts_greens_wide_body<T, true, 2>(smem, Bw, scr, M, nbins, first, Gd, Gd2, detd);
    }
};

// The quad engine (AFQ_THERMAL_QUAD, the complex walkers): the far placement with four columns per lane -- c, c + 64,
// c + 128 and c + 192 -- and every vector in LDS at 256 entries, so that the lanes hold M <= 256.  A column goes through
// the far engine's operations in the far engine's order (the four row-class sums added as tw_sum4 adds them, a lane's
// columns searched from the low one up with a strict >, then ts_wave_argmax): the far engine's bits where both run.
template <class T> struct TsQuad {
    static constexpr bool has_sweep = true;
    static size_t lds(int M) { return ts_greens_quad_lds<T>(M); }
    __host__ __device__ static size_t scratch(int M) { return ts_greens_far_scratch(M); }
    static const char *name(bool sweep) { return sweep ? "thermal_cgreens_quad_sweep_kernel" : "thermal_cgreens_quad_kernel"; }
    __device__ __forceinline__ static void body(unsigned char *smem, const T *Bw, T *scr, int M, int nbins, int first, T *Gd, T *Gd2, T *detd) {
        ts_greens_wide_body<T, true, 4>(smem, Bw, scr, M, nbins, first, Gd, Gd2, detd);
    }
};

// Every Green's launch of a handle, by the engine it was configured with (th_engine).  G and det of grid.x / 2 walkers
// from `stack`, the chain starting at bin `first` (src_w as TsGreensArgs has it), in the handle's own scratch; with Gs
// the sweep instead: grid (2 nw, bins), the bins from ts0 on into Gs, in the scratch Ts.
template <class T> int th_launch_greens(afq_handle *h, const T *stack, T *G, T *det, int first, int src_w, dim3 grid,
                                        T *Gs = nullptr, T *Ts = nullptr, int ts0 = 0) {
    const bool sweep = Gs != nullptr;
    const TsGreensArgs<T> a = {stack, G, det, sweep ? Ts : (T *)h->th_scratch, h->M, h->th_nbins, first, src_w, Gs, h->th_ss, ts0};
    if (h->th_engine == TH_ENGINE_WIDE) return ts_launch_greens<T, TsWide>(h, a, grid, sweep);
    if constexpr (std::is_same<T, cplx>::value) {                    // (the real walkers have no streamed, far or quad engine)
        if (h->th_engine == TH_ENGINE_QUAD) return ts_launch_greens<T, TsQuad>(h, a, grid, sweep);
        if (h->th_engine == TH_ENGINE_FAR) return ts_launch_greens<T, TsFar>(h, a, grid, sweep);
        if (h->th_engine == TH_ENGINE_STREAMED) return ts_launch_greens<T, TsStreamed>(h, a, grid, sweep);
    }
    return ts_launch_greens<T, TsResident>(h, a, grid, sweep);
}

// scalars of scratch per work-group of the handle's Green's kernel, whatever the walker kind: what the sweep of
// afq_thermal_estimates sizes its chunks from
inline size_t th_greens_scratch(const afq_handle *h) {
    return h->th_engine == TH_ENGINE_QUAD ? TsQuad<cplx>::scratch(h->M)
         : h->th_engine == TH_ENGINE_FAR ? TsFar<cplx>::scratch(h->M) : h->th_engine == TH_ENGINE_WIDE ? TsWide<cplx>::scratch(h->M)
         : h->th_engine == TH_ENGINE_STREAMED ? TsStreamed<cplx>::scratch(h->M) : (size_t)0;
}

// ---- the bound on M of a configure entry point

// One kernel's LDS as the refusal words it: "need <bytes(M)> bytes of LDS for <what>, a work-group has .. <hint>"
struct ThLds {
    const char *what;
    size_t (*bytes)(int M);
    const char *hint;
};

// M within what every kernel of `need` holds and within `lanes` columns (64: one per lane; TW_COLS: two; TQ_COLS: four); else the
// refusal "<who>: M = <M> <unit> ..." names the first that does not fit -- the columns before the kernels with
// lanes_first, behind them without -- with its bytes, and the largest M that passes.
inline int th_screen_bound(afq_handle *h, const std::string &who, const char *unit, int lanes, bool lanes_first,
                           std::initializer_list<ThLds> need) {
    auto fits = [&](int m) {
        for (const ThLds &k : need)
            if (k.bytes(m) > TH_LDS_MAX) return false;
        return m <= lanes;
    };
    const int M = h->M;
    if (fits(M)) return AFQ_OK;
    int mmax = M;
    while (mmax > 1 && !fits(mmax)) --mmax;
    const std::string head = who + ": M = " + std::to_string(M) + " " + unit + " ";
    const std::string tail = " (M <= " + std::to_string(mmax) + ")";
    const std::string columns = head + "are more than the " + (lanes == TQ_COLS ? std::to_string(TQ_COLS) + " columns of a wave, four per lane"
                                                                 : lanes == TW_COLS ? std::to_string(TW_COLS) + " columns of a wave, two per lane"
                                                                                 : std::to_string(lanes) + " lanes of a wave, one per column") + tail;
    if (lanes_first && M > lanes) AFQ_FAIL(h, AFQ_EUNSUPPORTED, columns);
    for (const ThLds &k : need)
        if (k.bytes(M) > TH_LDS_MAX)
            AFQ_FAIL(h, AFQ_EUNSUPPORTED, head + "need " + std::to_string(k.bytes(M)) + " bytes of LDS for " + k.what +
                     ", a work-group has " + std::to_string(TH_LDS_MAX) + tail + k.hint);
    AFQ_FAIL(h, AFQ_EUNSUPPORTED, columns);
}

// ---- the far route's kernels as th_screen_bound asks for them, and the bound they leave.  The two slice kernels are
// k_thermal_cplx.hip's; their LDS is stated here, beside the Green's kernel's, so that one place holds what the route
// keeps in LDS: no matrix.
inline size_t thc_slice_far_lds(int) { return 0; }                            // thermal_cslice_far_kernel: nothing
inline size_t thd_slice_far_lds(int) { return 2 * sizeof(double) * TW_COLS; } // thermal_cslice_dense_far_kernel: bv[128] of cplx
const ThLds THC_FAR_GREENS = {"the far Green's function (thermal_cgreens_far_kernel)", ts_greens_far_lds<cplx>, ""};
const ThLds THC_FAR_SLICE = {"the far slice kernel (thermal_cslice_far_kernel)", thc_slice_far_lds, ""};
const ThLds THD_FAR_SLICE = {"the far slice kernel (thermal_cslice_dense_far_kernel)", thd_slice_far_lds, ""};

// the largest M the far route admits: what th_screen_bound lets through with these kernels and TW_COLS columns
inline int th_far_bound() {
    int m = TW_COLS;
    while (m > 1 && (ts_greens_far_lds<cplx>(m) > TH_LDS_MAX || thc_slice_far_lds(m) > TH_LDS_MAX || thd_slice_far_lds(m) > TH_LDS_MAX)) --m;
    return m;
}

// ---- the quad route's kernels and its bound: the far route's reads and writes with every vector at TQ_COLS entries
inline size_t thc_slice_quad_lds(int) { return 0; }                            // thermal_cslice_quad_kernel: nothing
inline size_t thd_slice_quad_lds(int) { return 2 * sizeof(double) * TQ_COLS; } // thermal_cslice_dense_quad_kernel: bv[256] of cplx
static_assert(TQ_COLS <= TH_THREADS, "bv, a column exchange and a reflector load work one thread per entry: M <= TH_THREADS");
const ThLds THC_QUAD_GREENS = {"the quad Green's function (thermal_cgreens_quad_kernel)", ts_greens_quad_lds<cplx>, ""};
const ThLds THC_QUAD_SLICE = {"the quad slice kernel (thermal_cslice_quad_kernel)", thc_slice_quad_lds, ""};
const ThLds THD_QUAD_SLICE = {"the quad slice kernel (thermal_cslice_dense_quad_kernel)", thd_slice_quad_lds, ""};

inline int th_quad_bound() {
    int m = TQ_COLS;
    while (m > 1 && (ts_greens_quad_lds<cplx>(m) > TH_LDS_MAX || thc_slice_quad_lds(m) > TH_LDS_MAX || thd_slice_quad_lds(m) > TH_LDS_MAX)) --m;
    return m;
}

}  // namespace
