// The stratified Green's function of a finite-temperature walker, once for both walker kinds: T = double for the
// discrete Hirsch fields of k_thermal.hip, T = cplx for the continuous fields of k_thermal_cplx.hip.
//
//   thermal_greens_kernel<T, E, SWEEP>  the one kernel of every engine E.  One work-group per (walker, spin):
//                             G = [I + B_L .. B_1]^-1 from the stack by the stratified (graded) decomposition.
//                             Q D T = B_first by column-pivoted QR with Householder
//                             reflectors H = I - tau v v^H (alpha = -x_0 / |x_0| ||x||, tau = (||x|| + |x_0|) / ||x||
//                             real); for every further bin C = (B Q) D, Q D t = C, T <- t T; then with D = D_b^-1 D_s
//                             split at |D| = 1 (D_b = 1 / |D|, D_s = D / |D| where |D| > 1)
//                               G^-1 = I + Q D T = Q D_b^-1 (D_b Q^H + D_s T)   =>   (D_b Q^H + D_s T) G = D_b Q^H,
//                             one pivoted solve (the same G as T^-1 (D_b Q^H T^-1 + D_s)^-1 D_b Q^H without forming
//                             T^-1).  The products B Q and t T are fp64 MFMA (v_mfma_f64_16x16x4, one real product per
//                             step for double and four for cplx, tiles padded by zero operands); the Householder panels
//                             and the pivot search are plain wave code.  det G, where asked for, is the product of the
//                             pivots of an LU with partial pivoting of a copy of G in the matrix the solve has used up.
//                             SWEEP: the same work on a grid (2 nw, bins): work-group (x, y) makes G of (walker, spin) x
//                             at slice_ix = (ts0 + y) stack_size into a scratch [bins, nw, 2, M, M] -- the averaged
//                             estimators' sweep of afq_thermal_estimates, one launch whatever the number of bins.
//   thermal_rdm_kernel<T>     P_s = I - G_s^T as c128 for the force bias and the energy, nav = Re(tr P_up + tr P_down).
//
// An engine says where the chain's matrices live, what that costs in LDS and in device scratch, and what the launch is
// called in the trace (the names are per walker kind and engine, not per template: the benchmarks key on them):
//   TsResident<T>   ts_greens_body with W, Qt, T and t in LDS: 4 matrices of pitch M | 1 in units of T, which the
//                   160 KiB of a compute unit hold up to M = 64 for double and M = 47 for cplx.
//                   thermal_greens_kernel / thermal_cgreens_kernel, .._sweep_kernel.
//   TsStreamed<cplx>  the same ts_greens_body with T in device memory and t read out of W: 2 matrices in LDS, which
//                   hold a complex walker to M = 64 (117,536 B at the M = 57 shell).  AFQ_THERMAL_STREAMED_GREENS; the
//                   same bits as the resident placement.  thermal_cgreens_streamed_kernel, .._streamed_sweep_kernel.
//                   There is no TsStreamed<double>: the real walkers fit to M = 64 as they are.
//   TsWide<T>       (thermal_wide.h) another body, ts_greens_wide_body: one matrix in LDS and two columns per lane;
//                   the same G to rounding.  AFQ_THERMAL_WIDE: a complex walker to M = 95; AFQ_THERMAL_DELAYED: a real
//                   walker to M = 128.  thermal_cgreens_wide_kernel / thermal_greens_wide_kernel, .._sweep_kernel
//                   (afq_thermal_estimates still refuses AVERAGE_GF on the handles of these two bits: only TsFar's runs).
//   TsFar<T>        (thermal_wide.h) ts_greens_wide_body with its one matrix in the work-group's scratch as well: no
//                   matrix in LDS, the bits of TsWide.  AFQ_THERMAL_FAR: a complex walker to M = 128.
//                   thermal_cgreens_far_kernel, thermal_cgreens_far_sweep_kernel.
//   TsQuad<cplx>    (thermal_wide.h) TsFar's placement with four columns per lane: the bits of TsFar to M = 128.
//                   AFQ_THERMAL_QUAD: a complex walker to M = 256.  thermal_cgreens_quad_kernel, .._quad_sweep_kernel.
// th_launch is the one way a thermal kernel with dynamic LDS is launched; ts_launch_greens<T, E> the one launcher of the
// Green's kernels; th_launch_greens<T> (thermal_wide.h) picks E by the handle's th_engine.
//
// TsScalar<T> is the arithmetic the routines are written in.  Restricted to real numbers the complex formulas round as
// the real ones do: a product with +-1 and a negation are exact, so alpha = -unit(x_0) ||x||, x_0 - alpha =
// unit(x_0) (|x_0| + ||x||) and tau = (||x|| + |x_0|) / ||x|| are the doubles of alpha = x_0 >= 0 ? -||x|| : ||x|| and
// (alpha - x_0) / alpha.
#pragma once
#include "afq_internal.h"
#include "afq_host.h"
#include "mfma_gemm.h"
#include <cmath>
#include <type_traits>

#define TH_THREADS 256
#define TH_LDS_MAX (160 * 1024)

namespace {

template <class T> struct TsScalar;

template <> struct TsScalar<double> {
    typedef d4_t Acc;                                   // one MFMA accumulator
    __device__ static double zero() { return 0.0; }
    __device__ static double real(double r) { return r; }
    __device__ static double &re(double &a) { return a; }
    __device__ static double re(const double &a) { return a; }
    __device__ static cplx c128(double a) { return cmake(a, 0.0); }
    __device__ static double conj(double a) { return a; }
    __device__ static double abs(double a) { return fabs(a); }
    __device__ static double unit(double a, double) { return a >= 0.0 ? 1.0 : -1.0; }      // (-0.0 counts as +)
    __device__ static bool is_zero(double a) { return a == 0.0; }
    __device__ static double mul(double a, double b) { return a * b; }
    __device__ static double scale(double a, double s) { return a * s; }
    __device__ static double div(double a, double b) { return a / b; }
    __device__ static double neg(double a) { return -a; }
    __device__ static double add(double a, double b) { return a + b; }
    __device__ static void fma(double &a, double b, double c) { a = ::fma(b, c, a); }      // a += b c
    __device__ static void abs2(double &s, double a) { s = ::fma(a, a, s); }               // s += |a|^2
    __device__ static Acc acc0() { return (d4_t){0, 0, 0, 0}; }
    __device__ static void mma(Acc &c, double a, double b) { c = mfma16(a, b, c); }
    __device__ static double at(const Acc &c, int r) { return c[r]; }
};

template <> struct TsScalar<cplx> {
    struct Acc { d4_t re, im; };
    __device__ static cplx zero() { return cmake(0.0, 0.0); }
    __device__ static cplx real(double r) { return cmake(r, 0.0); }
    __device__ static double &re(cplx &a) { return a.x; }
    __device__ static double re(const cplx &a) { return a.x; }
    __device__ static cplx c128(cplx a) { return a; }
    __device__ static cplx conj(cplx a) { return cconj(a); }
    __device__ static double abs(cplx a) { return hypot(a.x, a.y); }
    __device__ static cplx unit(cplx a, double abs_a) { return cmake(a.x / abs_a, a.y / abs_a); }
    __device__ static bool is_zero(cplx a) { return a.x == 0.0 && a.y == 0.0; }
    __device__ static cplx mul(cplx a, cplx b) { return cmul(a, b); }
    __device__ static cplx scale(cplx a, double s) { return cscale(a, s); }
    __device__ static cplx div(cplx a, cplx b) { return cdiv(a, b); }
    __device__ static cplx neg(cplx a) { return cmake(-a.x, -a.y); }
    __device__ static cplx add(cplx a, cplx b) { return cadd(a, b); }
    __device__ static void fma(cplx &a, cplx b, cplx c) { cfma(a, b, c); }
    __device__ static void abs2(double &s, cplx a) { s = ::fma(a.x, a.x, s); s = ::fma(a.y, a.y, s); }
    __device__ static Acc acc0() { return {(d4_t){0, 0, 0, 0}, (d4_t){0, 0, 0, 0}}; }
    __device__ static void mma(Acc &c, cplx a, cplx b) {
        c.re = mfma16(a.x, b.x, c.re);
        c.re = mfma16(-a.y, b.y, c.re);
        c.im = mfma16(a.x, b.y, c.im);
        c.im = mfma16(a.y, b.x, c.im);
    }
    __device__ static cplx at(const Acc &c, int r) { return cmake(c.re[r], c.im[r]); }
};

// C = A B for M x M operands given as element loaders, by the 4 waves of the work-group: 16 x 16 tiles, k in steps of
// 4; rows, columns and k beyond M enter as zeros and are not stored.  The caller synchronises before and after.
template <class T, class LA, class LB, class ST>
__device__ inline void ts_gemm(int M, LA la, LB lb, ST st) {
    typedef TsScalar<T> S;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const int nt = (M + 15) >> 4, lr = lane & 15, lk = lane >> 4;
    for (int tile = wave; tile < nt * nt; tile += nwave) {
        const int row0 = (tile / nt) << 4, col0 = (tile % nt) << 4;
        const int arow = row0 + lr, bcol = col0 + lr;
        typename S::Acc acc = S::acc0();
        for (int k0 = 0; k0 < M; k0 += 4) {
            const int k = k0 + lk;
            const T a = (arow < M && k < M) ? la(arow, k) : S::zero();
            const T b = (bcol < M && k < M) ? lb(k, bcol) : S::zero();
            S::mma(acc, a, b);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + lk + 4 * r;
            if (row < M && bcol < M) st(row, bcol, S::at(acc, r));
        }
    }
}

// (value, index) of the largest val over the 64 lanes of a wave; ties go to the lower index; every lane gets the result
__device__ inline void ts_wave_argmax(double &val, int &idx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(val, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ov > val || (ov == val && oi < idx)) { val = ov; idx = oi; }
    }
}

template <class T> __device__ inline T ts_sum4(const T *p) {
    typedef TsScalar<T> S;
    return S::add(S::add(p[0], p[64]), S::add(p[128], p[192]));
}

// Column-pivoted Householder QR of W [M, M] (LDS, row-major, leading dimension LD), in place: W P = Q R.  On return
// the upper triangle of W holds R (zeros below), perm[j] the original column now at position j, Qt = Q^H.
// The pivot of step j is the remaining column of the largest norm over the rows j.., recomputed every step (no
// downdating).  part: 8 * 64 scalars, v: 64 scalars.  Every wave runs the pivot search on its own: no shared scalars.
template <class T> __device__ void ts_qrcp(T *W, T *Qt, int M, int LD, int *perm, T *v, T *part) {
    typedef TsScalar<T> S;
    const int tid = threadIdx.x, c = tid & 63, q = tid >> 6;
    for (int e = tid; e < M * M; e += TH_THREADS) { const int r = e / M, cc = e % M; Qt[r * LD + cc] = S::real(r == cc ? 1.0 : 0.0); }
    if (tid < M) perm[tid] = tid;
    __syncthreads();
    for (int j = 0; j < M; ++j) {
        if (c >= j && c < M) {
            double s = 0.0;
            for (int i = j + q; i < M; i += 4) S::abs2(s, W[i * LD + c]);
            S::re(part[q * 64 + c]) = s;
        }
        __syncthreads();
        double nrm2 = (c >= j && c < M) ? (S::re(part[c]) + S::re(part[64 + c])) + (S::re(part[128 + c]) + S::re(part[192 + c])) : -1.0;
        int piv = c;
        ts_wave_argmax(nrm2, piv);
        if (piv != j) {
            if (tid < M) { const T t = W[tid * LD + j]; W[tid * LD + j] = W[tid * LD + piv]; W[tid * LD + piv] = t; }
            if (tid == TH_THREADS - 1) { const int t = perm[j]; perm[j] = perm[piv]; perm[piv] = t; }
        }
        __syncthreads();
        const T x0 = W[j * LD + j];
        const double nrm = sqrt(nrm2), ax0 = S::abs(x0);
        const T ph = ax0 > 0.0 ? S::unit(x0, ax0) : S::real(1.0);
        const T alpha = S::scale(S::neg(ph), nrm);                   // H x = alpha e_0, |x_0 - alpha| = |x_0| + ||x||
        const double tau = nrm > 0.0 ? (nrm + ax0) / nrm : 0.0;
        const T den = S::scale(ph, ax0 + nrm);                       // x_0 - alpha, no cancellation
        if (tid < M - j)
            v[j + tid] = (tid == 0 || !(nrm > 0.0)) ? S::real(tid == 0 ? 1.0 : 0.0) : S::div(W[(j + tid) * LD + j], den);
        __syncthreads();
        // v^H W[:, c] for the trailing columns and v^H Qt[:, c] for every column, four row classes per column
        if (c < M) {
            T sw = S::zero(), sq = S::zero();
            for (int i = j + q; i < M; i += 4) {
                const T vc = S::conj(v[i]);
                if (c > j) S::fma(sw, vc, W[i * LD + c]);
                S::fma(sq, vc, Qt[i * LD + c]);
            }
            part[q * 64 + c] = sw; part[256 + q * 64 + c] = sq;
        }
        __syncthreads();
        if (c < M) {
            const T sw = S::scale(ts_sum4(part + c), -tau), sq = S::scale(ts_sum4(part + 256 + c), -tau);
            for (int i = j + q; i < M; i += 4) {
                const T vi = v[i];
                if (c > j) S::fma(W[i * LD + c], sw, vi);
                S::fma(Qt[i * LD + c], sq, vi);
            }
            if (c == j && nrm > 0.0) for (int i = j + q; i < M; i += 4) W[i * LD + j] = i == j ? alpha : S::zero();
        }
        __syncthreads();
    }
}

// X G = R for X, R [M, M] in LDS by Gauss-Jordan elimination with partial (row) pivoting; G overwrites R, X is
// destroyed.  colv, rowx, rowr: 64 scalars each.
template <class T> __device__ void ts_solve(T *X, T *R, int M, int LD, T *colv, T *rowx, T *rowr) {
    typedef TsScalar<T> S;
    const int tid = threadIdx.x, c = tid & 63;
    for (int k = 0; k < M; ++k) {
        double a = (c >= k && c < M) ? S::abs(X[c * LD + k]) : -1.0;
        int p = c;
        ts_wave_argmax(a, p);
        __syncthreads();                                  // (every wave has read column k before rows move)
        if (p != k) {
            if (tid < M) { const T t = X[k * LD + tid]; X[k * LD + tid] = X[p * LD + tid]; X[p * LD + tid] = t; }
            else if (tid >= 64 && tid < 64 + M) { const T t = R[k * LD + c]; R[k * LD + c] = R[p * LD + c]; R[p * LD + c] = t; }
        }
        __syncthreads();
        const T piv = X[k * LD + k];
        __syncthreads();
        if (tid < M) { colv[tid] = X[tid * LD + k]; rowx[tid] = S::div(X[k * LD + tid], piv); }
        else if (tid >= 64 && tid < 64 + M) rowr[c] = S::div(R[k * LD + c], piv);
        __syncthreads();
        for (int e = tid; e < M * M; e += TH_THREADS) {
            const int i = e / M, cc = e % M;
            if (i == k) { X[i * LD + cc] = rowx[cc]; R[i * LD + cc] = rowr[cc]; }
            else {
                const T f = S::neg(colv[i]);
                S::fma(X[i * LD + cc], f, rowx[cc]);
                S::fma(R[i * LD + cc], f, rowr[cc]);
            }
        }
        __syncthreads();
    }
}

// det X of X [M, M] in LDS: the product of the pivots of an LU with partial (row) pivoting, the sign of every row
// exchange included; X is destroyed.  Every thread returns the same value.  colv: 64 scalars.
template <class T> __device__ T ts_det(T *X, int M, int LD, T *colv) {
    typedef TsScalar<T> S;
    const int tid = threadIdx.x, c = tid & 63;
    T det = S::real(1.0);
    for (int k = 0; k < M; ++k) {
        double a = (c >= k && c < M) ? S::abs(X[c * LD + k]) : -1.0;
        int p = c;
        ts_wave_argmax(a, p);
        __syncthreads();
        if (p != k) {
            if (tid < M) { const T t = X[k * LD + tid]; X[k * LD + tid] = X[p * LD + tid]; X[p * LD + tid] = t; }
            det = S::neg(det);
        }
        __syncthreads();
        const T piv = X[k * LD + k];                      // (the same value in every thread: uniform branches below)
        det = S::mul(det, piv);
        if (S::is_zero(piv)) return S::zero();
        if (tid > k && tid < M) colv[tid] = S::div(X[tid * LD + k], piv);
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

__host__ __device__ inline size_t ts_mat(int M) { return (size_t)M * (M | 1); }
// first bin of the chain for the Green's function at slice_ix (walkers/thermal.py:477-492)
__host__ __device__ inline int ts_first_of(int slice_ix, int stack_size, int nbins) {
    int bin_ix = slice_ix / stack_size;
    if (bin_ix == nbins) bin_ix = -1;
    return (bin_ix + 1) % nbins;
}

// A matrix where a placement keeps it: LDS at pitch M | 1, or the work-group's scratch in device memory at pitch M
template <class T> struct TsMatView {
    T *p; int ld;
    __device__ T &operator()(int r, int c) const { return p[r * ld + c]; }
};

// LDS of the resident placement: 4 matrices, D[64], v[64], part[512], aux[192] scalars, perm[64]
template <class T> inline size_t ts_greens_lds(int M) { return sizeof(T) * (4 * ts_mat(M) + 64 + 64 + 512 + 192) + sizeof(int) * 64; }
// LDS of the streamed placement: W and Qt, and the same vectors
template <class T> inline size_t ts_greens_streamed_lds(int M) { return sizeof(T) * (2 * ts_mat(M) + 64 + 64 + 512 + 192) + sizeof(int) * 64; }

// The work of one work-group: G of one (walker, spin) from its bins Bw (bin b at Bw + b * 2 * M * M) in the order first,
// first + 1, .. (mod nbins), into Gd [M, M] and, where given, into Gd2 as well; det G into *detd where given.  P places
// the matrices (TsResident, TsStreamed below); scr: the work-group's own P::scratch(M) scalars of device memory.  Every
// element goes through the same operations in the same order whatever P is, so the placements give the same bits; a
// work-group reads from device memory only what it has written itself, across a __syncthreads().
template <class T, class P>
__device__ __forceinline__ void ts_greens_body(unsigned char *smem, const T *Bw, T *scr, int M, int nbins, int first, T *Gd,
                                               T *Gd2, T *detd) {
    typedef TsScalar<T> S;
    const int LD = M | 1, tid = threadIdx.x;
    P pl(smem, scr, M);
    T *W = pl.W, *const Qt = pl.Qt;                                  // LDS: the QR sweeps them four times per column
    TsMatView<T> Tc = pl.Tcur, Tn = pl.Tnext;                        // T and the result of t T, used in turn
    T *const D = pl.vec, *const v = D + 64, *const part = v + 64, *const aux = part + 512;
    int *const perm = (int *)(aux + 192);
    int *const iperm = (int *)aux;                                   // (aux is the solve's: free until the chain is done)
    const long mm = (long)M * M;

    {
        const T *B = Bw + (long)first * 2 * mm;
        for (int e = tid; e < M * M; e += TH_THREADS) W[(e / M) * LD + e % M] = B[e];
    }
    __syncthreads();
    ts_qrcp(W, Qt, M, LD, perm, v, part);
    // T = D^-1 R P^T
    for (int e = tid; e < M * M; e += TH_THREADS) {
        const int i = e / M, j = e % M;
        Tc(i, perm[j]) = j >= i ? S::div(W[i * LD + j], W[i * LD + i]) : S::zero();
    }
    if (tid < M) D[tid] = W[tid * LD + tid];
    __syncthreads();
    for (int n = 1; n < nbins; ++n) {
        const T *B = Bw + (long)((first + n) % nbins) * 2 * mm;
        // W = (B Q) D, Q[k][c] = conj(Qt[c][k])
        ts_gemm<T>(M, [&](int r, int k) { return B[r * M + k]; }, [&](int k, int c) { return S::conj(Qt[c * LD + k]); },
                   [&](int r, int c, T x) { W[r * LD + c] = S::mul(x, D[c]); });
        __syncthreads();
        ts_qrcp(W, Qt, M, LD, perm, v, part);
        // t = D^-1 R P^T: stored in LDS where the placement has the room, else read out of W through the inverse
        // permutation by the loader of t T
        if constexpr (P::stores_t) {
            for (int e = tid; e < M * M; e += TH_THREADS) {
                const int i = e / M, j = e % M;
                pl.X[i * LD + perm[j]] = j >= i ? S::div(W[i * LD + j], W[i * LD + i]) : S::zero();
            }
        } else if (tid < M) iperm[perm[tid]] = tid;
        if (tid < M) D[tid] = W[tid * LD + tid];
        __syncthreads();
        // T <- t T
        ts_gemm<T>(M, [&](int r, int k) {
                       if constexpr (P::stores_t) return pl.X[r * LD + k];
                       else { const int j = iperm[k]; return j >= r ? S::div(W[r * LD + j], W[r * LD + r]) : S::zero(); }
                   },
                   [&](int k, int c) { return Tc(k, c); }, [&](int r, int c, T x) { Tn(r, c) = x; });
        __syncthreads();
        pl.turn(W, Tc, Tn);
    }
    // (D_b Q^H + D_s T) G = D_b Q^H, D_b = 1 / |D| and D_s = D / |D| where |D| > 1, else D_b = 1 and D_s = D
    T *const X = pl.solve_x(W), *const R = pl.solve_rhs(W);
    for (int e = tid; e < M * M; e += TH_THREADS) {
        const int i = e / M, j = e % M;
        const T d = D[i];
        const double ad = S::abs(d);
        const double db = ad > 1.0 ? 1.0 / ad : 1.0;
        const T ds = ad > 1.0 ? S::unit(d, ad) : d;
        const T r = S::scale(Qt[i * LD + j], db);
        T x = r;
        S::fma(x, ds, Tc(i, j));
        X[i * LD + j] = x;
        R[i * LD + j] = r;
    }
    __syncthreads();
    ts_solve(X, R, M, LD, aux, aux + 64, aux + 128);
    // (only the complex walkers carry determinants: the real kernel holds no code for them)
    const bool want_det = std::is_same<T, cplx>::value && detd;
    for (int e = tid; e < M * M; e += TH_THREADS) {
        const T g = R[(e / M) * LD + e % M];
        Gd[e] = g;
        if (Gd2) Gd2[e] = g;
        if (want_det) X[(e / M) * LD + e % M] = g;
    }
    if (!want_det) return;
    __syncthreads();
    const T dg = ts_det(X, M, LD, aux);
    if (tid == 0) *detd = dg;
}

// The resident engine: W, Qt, T and X (t of the chain, then the matrix of the closing solve) in LDS.  t T goes into W,
// whose R is used up, and the two change names; the solve's right-hand side D_b Q^H is built in the W of the end.
template <class T> struct TsResident {
    static constexpr bool stores_t = true, has_sweep = true;
    static size_t lds(int M) { return ts_greens_lds<T>(M); }
    __host__ __device__ static size_t scratch(int) { return 0; }
    static const char *name(bool sweep) {
        return std::is_same<T, cplx>::value ? (sweep ? "thermal_cgreens_sweep_kernel" : "thermal_cgreens_kernel")
                                            : (sweep ? "thermal_greens_sweep_kernel" : "thermal_greens_kernel");
    }
    T *W, *Qt, *X, *vec;
    TsMatView<T> Tcur, Tnext;
    __device__ TsResident(unsigned char *smem, T *, int M) {
        const size_t mat = ts_mat(M);
        W = (T *)smem; Qt = W + mat; Tcur = {Qt + mat, M | 1}; X = Tcur.p + mat; vec = X + mat;
        Tnext = {W, M | 1};
    }
    __device__ void turn(T *&w, TsMatView<T> &tc, TsMatView<T> &tn) const { w = tc.p; tc.p = tn.p; tn.p = w; }
    __device__ T *solve_x(T *) const { return X; }
    __device__ T *solve_rhs(T *w) const { return w; }
    __device__ __forceinline__ static void body(unsigned char *smem, const T *Bw, T *scr, int M, int nbins, int first, T *Gd, T *Gd2, T *detd) {
        ts_greens_body<T, TsResident<T>>(smem, Bw, scr, M, nbins, first, Gd, Gd2, detd);
    }
};

// The streamed engine: W and Qt stay in LDS; T, touched once per bin as the B operand and the result of t T, lives in
// the work-group's own scratch, two [M, M] buffers of pitch M used in turn; t is never stored.  The closing solve runs
// in the two LDS matrices: D_b Q^H in place in Qt, its matrix in W.  The complex walkers' alone.
template <class T> struct TsStreamed;
template <> struct TsStreamed<cplx> {
    static constexpr bool stores_t = false, has_sweep = true;
    static size_t lds(int M) { return ts_greens_streamed_lds<cplx>(M); }
    __host__ __device__ static size_t scratch(int M) { return 2 * (size_t)M * M; }
    static const char *name(bool sweep) { return sweep ? "thermal_cgreens_streamed_sweep_kernel" : "thermal_cgreens_streamed_kernel"; }
    cplx *W, *Qt, *X = nullptr, *vec;
    TsMatView<cplx> Tcur, Tnext;
    __device__ TsStreamed(unsigned char *smem, cplx *scr, int M) {
        const size_t mat = ts_mat(M);
        W = (cplx *)smem; Qt = W + mat; vec = Qt + mat;
        Tcur = {scr, M}; Tnext = {scr + (long)M * M, M};
    }
    __device__ void turn(cplx *&, TsMatView<cplx> &tc, TsMatView<cplx> &tn) const { cplx *t = tc.p; tc.p = tn.p; tn.p = t; }
    __device__ cplx *solve_x(cplx *w) const { return w; }
    __device__ cplx *solve_rhs(cplx *) const { return Qt; }
    __device__ __forceinline__ static void body(unsigned char *smem, const cplx *Bw, cplx *scr, int M, int nbins, int first, cplx *Gd, cplx *Gd2,
                                cplx *detd) {
        ts_greens_body<cplx, TsStreamed<cplx>>(smem, Bw, scr, M, nbins, first, Gd, Gd2, detd);
    }
};

// What a Green's launch works on.  One Green's function per (walker, spin), grid (nblocks): with src_w < 0 block b works
// on walker b / 2, otherwise every block works on walker src_w and writes walker 0's place (grid of 2 blocks); the chain
// starts at bin `first`.  The sweep, grid (2 nw, bins): work-group (x, y) makes G of (walker, spin) x at slice_ix =
// (ts0 + y) stack_size, for every y at once, into Gs [gridDim.y, nw, 2, M, M]; the last bin of the path
// (ts = nbins - 1) also goes to the walkers' own G and det: what afq_thermal_greens leaves there.
template <class T> struct TsGreensArgs {
    const T *stack;             // [nw, nbins, 2, M, M]
    T *G, *det;                 // [nw, 2, M, M], [nw, 2]; det may be null (and is, for the real walkers)
    T *scratch;                 // [work-groups, E::scratch(M)]: every work-group its own (null for the resident engine)
    int M, nbins;
    int first, src_w;           // one Green's function per (walker, spin)
    T *Gs;                      // the sweep
    int stack_size, ts0;
};

template <class T, template <class> class E, bool SWEEP>
__global__ __launch_bounds__(TH_THREADS) void thermal_greens_kernel(TsGreensArgs<T> a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int M = a.M, s = blockIdx.x & 1;
    const long mm = (long)M * M;
    if (SWEEP) {
        const int w = blockIdx.x >> 1, ts = a.ts0 + (int)blockIdx.y;
        const long slot = (long)w * 2 + s, wg = (long)blockIdx.y * gridDim.x + blockIdx.x;
        const bool last = ts == a.nbins - 1;
        E<T>::body(smem, a.stack + ((long)w * a.nbins * 2 + s) * mm, a.scratch + wg * (long)E<T>::scratch(M), M, a.nbins,
                   ts_first_of(ts * a.stack_size, a.stack_size, a.nbins), a.Gs + wg * mm, last ? a.G + slot * mm : nullptr,
                   last && a.det ? a.det + slot : nullptr);
    } else {
        const int w = a.src_w < 0 ? blockIdx.x >> 1 : a.src_w;
        const long slot = (long)(a.src_w < 0 ? w : 0) * 2 + s;
        E<T>::body(smem, a.stack + ((long)w * a.nbins * 2 + s) * mm, a.scratch + (long)blockIdx.x * (long)E<T>::scratch(M), M,
                   a.nbins, a.first, a.G + slot * mm, nullptr, a.det ? a.det + slot : nullptr);
    }
}

// P_s = I - G_s^T as c128 [nw, 2, M, M], nav = Re(tr P_up + tr P_down) (nav may be null)
template <class T>
__global__ __launch_bounds__(TH_THREADS) void thermal_rdm_kernel(const T *G, cplx *P, double *nav, int M) {
    typedef TsScalar<T> S;
    __shared__ double red[TH_THREADS];
    const int w = blockIdx.x, tid = threadIdx.x;
    const long mm = (long)M * M;
    const T *Gw = G + (long)w * 2 * mm;
    cplx *Pw = P + (long)w * 2 * mm;
    for (int e = tid; e < 2 * M * M; e += TH_THREADS) {
        const int s = e / (M * M), r = (e / M) % M, c = e % M;
        T p = S::neg(Gw[s * mm + (long)c * M + r]);
        S::re(p) += r == c ? 1.0 : 0.0;
        Pw[e] = S::c128(p);
    }
    if (!nav) return;
    double t = 0.0;
    for (int e = tid; e < 2 * M; e += TH_THREADS) t += 1.0 - S::re(Gw[(e / M) * mm + (long)(e % M) * M + e % M]);
    red[tid] = t;
    __syncthreads();
    for (int o = TH_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) nav[w] = red[0];
}

// what every thermal entry point asks first; want_cplx: the continuous fields' walkers are needed
inline int th_need(afq_handle *h, bool want_cplx) {
    if (!th_thermal(h) || !h->nw || (want_cplx && !th_complex(h)))
        AFQ_FAIL(h, AFQ_ESTATE, want_cplx ? "thermal walkers: afq_thermal_configure_continuous or afq_thermal_configure_hubbard_continuous first"
                                          : "thermal walkers: afq_thermal_configure or afq_thermal_configure_continuous first");
    if (h->prop_pending) AFQ_FAIL(h, AFQ_ESTATE, "a step is half done: afq_propagate_finish first");
    hipSetDevice(h->device);
    return AFQ_OK;
}

// ---- what the three configure entry points refuse alike, in the order they refuse it.  An entry point words a few of
// the refusals its own way: those words are this description of it.
struct ThEntry {
    std::string me;             // "<entry point>: "
    int allowed;                // the option bits it takes
    int charge_code;            // AFQ_THERMAL_CHARGE: the error code and the text
    std::string charge_text;
    int system;                 // the AFQ_SYS_ kind it serves, and the refusal of another
    std::string system_text;
    const char *ge1;            // "all" / "both" of "(.. >= 1)"
};

// the option bits, then the system and the walkers; the entry point's own bound on M follows
inline int th_screen_options(afq_handle *h, const ThEntry &e, int options) {
    if (options & AFQ_THERMAL_CHARGE) AFQ_FAIL(h, e.charge_code, e.charge_text);
    if (options & AFQ_THERMAL_FREE_PROJECTION) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: free_projection is not supported (constrained path only)");
    if (options & AFQ_THERMAL_LOW_RANK) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: low_rank is not supported");
    if (options & AFQ_THERMAL_AVERAGE_GF) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: average_gf is not supported");
    if (options & AFQ_THERMAL_STREAMED_GREENS & ~e.allowed)
        AFQ_FAIL(h, AFQ_EINVAL, e.me + "streamed_greens belongs to the continuous fields (the real walkers fit to M = 64 as they are)");
    if (options & AFQ_THERMAL_WIDE & ~e.allowed)
        AFQ_FAIL(h, AFQ_EINVAL, e.me + "wide_basis belongs to the continuous fields (the real walkers work one lane per column, M <= 64)");
    if (options & AFQ_THERMAL_FAR & ~e.allowed)
        AFQ_FAIL(h, AFQ_EINVAL, e.me + "far_basis belongs to the continuous fields (the real walkers reach M = 128 with delayed_updates)");
    if (options & AFQ_THERMAL_QUAD & ~e.allowed)
        AFQ_FAIL(h, AFQ_EINVAL, e.me + "quad_basis belongs to the continuous fields (the real walkers reach M = 128 with delayed_updates)");
    if (options & AFQ_THERMAL_DELAYED & ~e.allowed) AFQ_FAIL(h, AFQ_EINVAL, e.me + "delayed_updates belongs to the discrete fields");
    if (options & ~e.allowed) AFQ_FAIL(h, AFQ_EINVAL, e.me + "unknown option bits");
    if (!h->kind || !h->nw) AFQ_FAIL(h, AFQ_ESTATE, e.me + "set the system and allocate the walkers first");
    if (h->kind != e.system) AFQ_FAIL(h, AFQ_EUNSUPPORTED, e.system_text);
    return AFQ_OK;
}

// behind the bound on M: what else the handle is doing, and the shape of the path (nstblz: 1 where there is none)
inline int th_screen_state(afq_handle *h, const ThEntry &e, int ntime_slices, int stack_size, int nstblz) {
    if (k_comm_size(h) > 1) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: one rank only");
    if (h->nbp > 0 || h->it_nmax > 0) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: no back-propagation or ITCF window");
    if (h->rdm_on) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: no mixed one_rdm / two_rdm");
    if (ntime_slices < 1 || stack_size < 1 || nstblz < 1 || ntime_slices % stack_size)
        AFQ_FAIL(h, AFQ_EINVAL, e.me + "stack_size must divide ntime_slices (" + e.ge1 + " >= 1)");
    return AFQ_OK;
}

// PropagatorStack.update's counters behind a slice (stack.py:295-297, 322-324)
inline void th_advance(afq_handle *h) {
    h->th_slice += 1;
    h->th_block = h->th_slice / h->th_ss;
    h->th_counter = (h->th_counter + 1) % h->th_ss;
}

// first bin of the chain for the Green's function at slice_ix (walkers/thermal.py:477-492)
inline int ts_first_bin(const afq_handle *h, int slice_ix) { return ts_first_of(slice_ix, h->th_ss, h->th_nbins); }

// The one launch of a thermal kernel that takes dynamic LDS, TH_THREADS threads a work-group: the kernel's LDS attribute
// raised once per device, `name` into the launch trace, the launch on the handle's stream and its check.
template <auto Kern, class... Args> int th_launch(afq_handle *h, const char *name, dim3 grid, size_t lds, Args... args) {
    static size_t lds_set[AFQ_MAX_DEVICES] = {0};                    // (one per kernel: Kern is a template argument)
    AFQ_HIP(h, afq_raise_lds((const void *)Kern, lds, lds_set));
    afq_note_launch(h, name);
    hipLaunchKernelGGL(Kern, grid, dim3(TH_THREADS), lds, h->stream, args...);
    AFQ_POST(h);
    return AFQ_OK;
}

// The one launcher of the Green's kernels: LDS and the name in the trace are the engine's.  a.scratch holds
// E::scratch(M) scalars for every work-group of the grid.
template <class T, template <class> class E> int ts_launch_greens(afq_handle *h, const TsGreensArgs<T> &a, dim3 grid, bool sweep) {
    if constexpr (E<T>::has_sweep) {
        if (sweep) return th_launch<thermal_greens_kernel<T, E, true>>(h, E<T>::name(true), grid, E<T>::lds(a.M), a);
    }
    if (sweep) AFQ_FAIL(h, AFQ_EUNSUPPORTED, std::string(E<T>::name(false)) + " has no sweep");
    return th_launch<thermal_greens_kernel<T, E, false>>(h, E<T>::name(false), grid, E<T>::lds(a.M), a);
}

// P_s = I - G_s^T of n Green's functions G [n, 2, M, M] into P, nav [n] (or null): the sweep's own scratch
template <class T> int ts_launch_rdm_n(afq_handle *h, const T *G, cplx *P, double *nav, int n) {
    afq_note_launch(h, std::is_same<T, cplx>::value ? "thermal_crdm_kernel" : "thermal_rdm_kernel");
    hipLaunchKernelGGL(thermal_rdm_kernel<T>, dim3(n), dim3(TH_THREADS), 0, h->stream, G, P, nav, h->M);
    AFQ_POST(h);
    return AFQ_OK;
}

// P [nw, 2, M, M] into the handle's c128 G buffer, nav (or null) from the walkers' G
template <class T> int ts_launch_rdm(afq_handle *h, const T *G, double *nav) { return ts_launch_rdm_n<T>(h, G, h->G, nav, h->nw); }

// (E, T, V) of every walker as the real parts of the handle's c128 [3, nw] energies, and nav; either may be null
inline int th_energy_out(afq_handle *h, double *E_out, double *nav_out) {
    if (E_out) {
        std::vector<double> e(6 * (size_t)h->nw);
        AFQ_TRY(copy_out(h, e.data(), h->energy, sizeof(cplx) * 3 * (size_t)h->nw));
        for (size_t i = 0; i < 3 * (size_t)h->nw; ++i) E_out[i] = e[2 * i];
    }
    return copy_out(h, nav_out, h->th_nav, sizeof(double) * (size_t)h->nw);
}

}  // namespace
