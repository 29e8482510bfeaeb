// Finite-temperature AFQMC walkers with continuous Hubbard-Stratonovich fields for the uniform electron gas
// (thermal_propagation/planewave.py:219-276,445-517, walkers/stack.py:299-324, walkers/thermal.py:51-64,472-547 of the
// reference; phaseless path, force bias on, full-rank walkers, diagonal one-body trial density matrix).  Every matrix of
// the walker is complex: G_s c128 [2, M, M], the bins c128 [nbins, 2, M, M], the running product of the current bin
// `right` c128 [2, M, M] and M0_s = det G_s c128 [2].  The slice counter, the block and the in-bin counter are the
// handle's, as for the real walkers of k_thermal.hip.  A walker's working set stays in LDS: 4 complex matrices of pitch
// M | 1, which the 160 KiB of a compute unit hold up to M = 47 (the plane-wave shells: 7, 19, 27, 33; 57 does not fit).
// With AFQ_THERMAL_STREAMED_GREENS the Green's function keeps 2 matrices in LDS and T in the handle's th_scratch; the
// bound is then the slice kernel's three matrices: M = 57, the next shell.  81 is refused on both of these routes.
// With AFQ_THERMAL_WIDE the handle takes a third route: thermal_wide.h's engine and the wide instantiations of the two
// slice kernels below keep ONE complex matrix in LDS and the rest in th_scratch, and a lane owns two columns: M <= 95,
// which holds the shells of 81 and 93 plane waves and the Hubbard lattices to 9 x 9.
// With AFQ_THERMAL_FAR a fourth: the wide route with that one matrix in th_scratch as well -- thermal_wide.h's body with W
// as a fifth scratch buffer, and the far instantiations of the slice kernels, which read every operand where it lies in
// device memory -- so that the lanes alone bind: M <= 128, which holds the shell of 123 plane waves and the Hubbard
// lattices 10 x 10, 11 x 11 and 8 x 16.  The same bits as the wide route wherever both run.
// With AFQ_THERMAL_QUAD a fifth: the far route with four columns per lane (thermal_wide.h's TsQuad) and the far
// instantiations of the slice kernels launched under their own names, bv at 256 entries: M <= 256, which holds the shells to 251
// plane waves and the Hubbard lattices 12 x 12 and 16 x 16.  The same bits as the far route wherever both run.
// The route is the handle's th_engine: th_launch_greens<cplx> (thermal_wide.h) and the two slice launches read it, and
// nothing else does.  The names below are the launch trace's; each slice kernel is one template over where its matrices
// live (ThcPlace: all in LDS; one matrix in LDS and the rest in th_scratch; none in LDS).
//
//   thermal_cgreens_far_kernel, thermal_cslice_far_kernel, thermal_cslice_dense_far_kernel  the far route's three.
//   thermal_cgreens_quad_kernel, thermal_cslice_quad_kernel, thermal_cslice_dense_quad_kernel  the quad route's three.
//   thermal_cgreens_kernel  G and det G of every (walker, spin) from the stack: thermal_strat.h's engine with T = cplx.
//   thermal_cgreens_streamed_kernel  the same with the streamed placement, for a handle configured with the bit.
//   thermal_cgreens_wide_kernel  thermal_wide.h's engine, for a handle configured with AFQ_THERMAL_WIDE.
//   thermal_cslice_wide_kernel, thermal_cslice_dense_wide_kernel  the two slice kernels below with one matrix in LDS.
//   thermal_cslice_kernel   one work-group per walker: BV = sum_{n <= 6} VHS^n / n! by five Horner products in LDS,
//                           once for both spins; per spin B = diag(BH1) BV diag(BH1), right <- B right (right = I at
//                           in-bin counter 0), bin[block] = diag(left_k) right.
//   thermal_cweight_kernel  the phaseless weight update from the determinant ratio, per walker.
//   thermal_crdm_kernel     P_s = I - G_s^T for the force bias and the energy (thermal_strat.h).
//   thermal_cfields_kernel  clip, shifted fields, cmf and cfb of every walker, dead ones included.
// The force bias and the HS potential are the plane-wave kernels of k_models.hip on P.
//
// The same walkers serve the Hubbard model with continuous fields (afq_thermal_configure_hubbard_continuous;
// thermal_propagation/continuous.py with hubbard.py:199-250): a dense real trial density matrix, a dense real BH1 and a
// diagonal field exponential.  Green's function, P, reset and the comb are the ones above; its own are
//   thermal_cfields_dense_kernel  force bias from the diagonal of P (no GEMM), clip at 1, xs, cmf, cfb, bv = diag BV.
//   thermal_cslice_dense_kernel   per spin B = BH1 (BV BH1), right <- B right, bin[block] = left_k right with the dense
//                                 left_k of the host's table; BH1_s staged in LDS.  M <= 63 (LDS); with the resident
//                                 Green's function the bound stays 47.
//   thermal_cweight_mf_kernel     the weight update with the constant of the mean-field shift.
#include "thermal_strat.h"
#include "thermal_wide.h"
#include <cstring>

#define THC_LANES 64            // the engine works lane = column

namespace {

inline size_t thc_slice_lds(int M) { return sizeof(cplx) * 3 * ts_mat(M); }

struct ThcSliceArgs {
    const cplx *vhs;            // [nw, M, M]
    cplx *right, *stack;        // [nw, 2, M, M], [nw, nbins, 2, M, M]
    const double *bh1, *left;   // diagonals [2, M]: BH1, and left_k of the slice being added
    int M, nbins, block, counter;
};

// One matrix in LDS (AFQ_THERMAL_WIDE): V alone; the Horner iterates live in the walker's scratch in device memory
inline size_t thc_slice_wide_lds(int M) { return sizeof(cplx) * ts_mat(M); }
// (no matrix in LDS, AFQ_THERMAL_FAR: thc_slice_far_lds of thermal_wide.h -- V is read where k_vhs_ueg left it)

// Where a slice kernel keeps its matrices: all in LDS; one in LDS and the rest in the walker's scratch in device memory
// (the wide route); none in LDS (the far route)
enum ThcPlace { THC_IN_LDS, THC_ONE_IN_LDS, THC_NONE_IN_LDS };

// One work-group per walker.  V, the A operand of all five Horner products, is in LDS.  THC_IN_LDS: so are the Horner
// iterates T_n, two matrices of pitch M | 1 used in turn, and BV = T_1 is read where it is.  THC_ONE_IN_LDS (the wide
// route): the T_n live in two [M, M] buffers of the walker's scratch (scratch + w stride, pitch M; a work-group reads
// back only what it wrote, across a barrier), and behind the Horner chain BV takes V's place in LDS as the A operand of
// right <- B right.  THC_NONE_IN_LDS (the far route): the T_n in scratch as well, V read from a.vhs in device memory
// and BV from the scratch buffer the Horner chain leaves it in.  Every element goes through the same operations in the
// same order -- the same ts_gemm with other loaders -- so the instantiations give the same bits where they run.
// The quad route launches the THC_NONE_IN_LDS instantiation under its own name: the kernel keeps no vector, so nothing in
// it knows how many columns a lane of the Green's kernel owns.
template <ThcPlace P> __global__ __launch_bounds__(TH_THREADS) void thermal_cslice_kernel(ThcSliceArgs a, cplx *scratch, long stride) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr bool IN_LDS = P == THC_IN_LDS, FAR = P == THC_NONE_IN_LDS;
    const int M = a.M, LD = M | 1, tid = threadIdx.x, w = blockIdx.x;
    const size_t mat = ts_mat(M);
    const long mm = (long)M * M;
    cplx *V = (cplx *)smem;
    TsMatView<cplx> T1 = {V + mat, LD}, T2 = {V + 2 * mat, LD};
    if (!IN_LDS) { T1 = {scratch + (long)w * stride, M}; T2 = {T1.p + mm, M}; }
    const cplx *Vw = a.vhs + (long)w * mm;
    // Horner: T_6 = I + V / 6, T_n = I + V T_{n + 1} / n, BV = T_1
    for (int e = tid; e < M * M; e += TH_THREADS) {
        const int r = e / M, c = e % M;
        const cplx x = Vw[e];
        if (!FAR) V[r * LD + c] = x;
        T1(r, c) = cmake(x.x / 6.0 + (r == c ? 1.0 : 0.0), x.y / 6.0);
    }
    __syncthreads();
    for (int n = 5; n >= 1; --n) {
        const double dn = (double)n;
        ts_gemm<cplx>(M, [&](int r, int k) { return FAR ? Vw[r * M + k] : V[r * LD + k]; }, [&](int k, int c) { return T1(k, c); },
                 [&](int r, int c, cplx x) { T2(r, c) = cmake(x.x / dn + (r == c ? 1.0 : 0.0), x.y / dn); });
        __syncthreads();
        const TsMatView<cplx> t = T1; T1 = T2; T2 = t;
    }
    TsMatView<cplx> BV = T1;
    if (P == THC_ONE_IN_LDS) {
        for (int e = tid; e < M * M; e += TH_THREADS) V[(e / M) * LD + e % M] = T1.p[e];
        __syncthreads();
        BV = {V, LD};
    }
    for (int s = 0; s < 2; ++s) {
        const double *d = a.bh1 + s * M, *lf = a.left + s * M;
        cplx *R = a.right + ((long)w * 2 + s) * mm;
        cplx *S = a.stack + (((long)w * a.nbins + a.block) * 2 + s) * mm;
        // B = diag(d) (BV diag(d)) as the reference forms it; right <- B right, right = I at the start of a bin
        if (a.counter == 0) {
            for (int e = tid; e < M * M; e += TH_THREADS) {
                const int r = e / M, c = e % M;
                const cplx x = cscale(cscale(BV(r, c), d[c]), d[r]);
                R[e] = x;
                S[e] = cscale(x, lf[r]);
            }
            continue;
        }
        ts_gemm<cplx>(M, [&](int r, int k) { return cscale(cscale(BV(r, k), d[k]), d[r]); },
                 [&](int k, int c) { return R[k * M + c]; }, [&](int r, int c, cplx x) { T2(r, c) = x; });
        __syncthreads();
        for (int e = tid; e < M * M; e += TH_THREADS) {
            const int r = e / M, c = e % M;
            const cplx x = T2(r, c);
            R[e] = x;
            S[e] = cscale(x, lf[r]);
        }
        __syncthreads();
    }
}

// planewave.py:239-269 / continuous.py:97-115 for one field n of walker w, whatever the walker's weight: a component of
// xbar = b with |b| > fb_bound is scaled to unit modulus (counted in acc[6]), xs = xi - xbar, and the field's terms of
// xs . mf (acc[0, 1]), xi . xbar (acc[2, 3]) and xbar . xbar (acc[4, 5], unconjugated).  -> xs
__device__ __forceinline__ cplx thc_field_terms(cplx b, double fb_bound, double x, cplx m, long e, cplx *xbar, cplx *xs,
                                                double *acc) {
    const double ab = hypot(b.x, b.y);
    if (ab > fb_bound) { b.x /= ab; b.y /= ab; acc[6] += 1.0; }
    const cplx sft = cmake(x - b.x, -b.y);
    xbar[e] = b;
    xs[e] = sft;
    acc[0] += sft.x * m.x - sft.y * m.y;
    acc[1] += sft.x * m.y + sft.y * m.x;
    acc[2] += x * b.x; acc[3] += x * b.y;
    acc[4] += b.x * b.x - b.y * b.y;
    acc[5] += 2.0 * b.x * b.y;
    return sft;
}

// Every thread has summed its fields in order; the 256 partial sums are added in a fixed tree: the same bits on every
// run.  cmf = -sqrt(dt) xs . mf, cfb = xi . xbar - xbar . xbar / 2, the clipped components onto counters[0] (as the
// ground-state field kernel counts its own).
__device__ __forceinline__ void thc_field_sums(const double *acc, int w, double sqrt_dt, cplx *cmf, cplx *cfb,
                                               unsigned long long *counters) {
    __shared__ double red[7][TH_THREADS];
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < 7; ++q) red[q][tid] = acc[q];
    __syncthreads();
    for (int o = TH_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o)
#pragma unroll
            for (int q = 0; q < 7; ++q) red[q][tid] += red[q][tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        cmf[w] = cmake(-sqrt_dt * red[0][0], -sqrt_dt * red[1][0]);
        cfb[w] = cmake(red[2][0] - 0.5 * red[4][0], red[3][0] - 0.5 * red[5][0]);
        if (red[6][0] > 0 && counters) atomicAdd(&counters[0], (unsigned long long)red[6][0]);
    }
}

// planewave.py:239-269 for one walker per work-group: xbar = -sqrt(dt) vbias clipped at fb_bound, xs, cmf, cfb
__global__ __launch_bounds__(TH_THREADS) void thermal_cfields_kernel(const cplx *vbias, const double *xi, const cplx *mf,
                                                                       cplx *xbar, cplx *xs, cplx *cmf, cplx *cfb, int K,
                                                                       double sqrt_dt, double fb_bound,
                                                                       unsigned long long *counters) {
    const int w = blockIdx.x, tid = threadIdx.x;
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int n = tid; n < K; n += TH_THREADS) {
        const long e = (long)w * K + n;
        const cplx v = vbias[e];
        thc_field_terms(cmake(-sqrt_dt * v.x, -sqrt_dt * v.y), fb_bound, xi[e], mf[n], e, xbar, xs, acc);
    }
    thc_field_sums(acc, w, sqrt_dt, cmf, cfb, counters);
}

// planewave.py:493-517: oratio = M0_up M0_dn / (Mnew_up Mnew_dn), hyb = log(oratio) + cfb + cmf, magn = |exp(hyb)|, or
// with MF (continuous.py:234-257) |mfc exp(hyb)|, mfc the constant of the mean-field shift; a zero denominator or a magn
// that is not finite: weight 0 and M0 kept; else weight *= magn max(0, cos arg exp(hyb - cfb)) and M0 <- Mnew (also when
// the cosine factor is 0).
template <bool MF>
__device__ __forceinline__ void thc_weight_update(double *weight, cplx *M0, const cplx *Mnew, const cplx *cmf, const cplx *cfb,
                                                  cplx mfc, int nw) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    const cplx num = cmul(M0[2 * w], M0[2 * w + 1]), den = cmul(Mnew[2 * w], Mnew[2 * w + 1]);
    if (den.x == 0.0 && den.y == 0.0) { weight[w] = 0.0; return; }
    const cplx oratio = cdiv(num, den);
    const cplx lg = cmake(log(hypot(oratio.x, oratio.y)), atan2(oratio.y, oratio.x));
    const cplx hyb = cadd(cadd(lg, cfb[w]), cmf[w]);
    double magn = exp(hyb.x);
    if (MF) {
        const cplx eq = cmul(mfc, cmake(magn * cos(hyb.y), magn * sin(hyb.y)));
        magn = hypot(eq.x, eq.y);
    }
    if (!(magn < INFINITY)) { weight[w] = 0.0; return; }      // infinite or NaN (a NaN M0 or Mnew): dies, keeps M0
    const double dtheta = hyb.y - cfb[w].y;
    const double cosine = fmax(0.0, cos(dtheta));
    weight[w] *= magn * cosine;
    M0[2 * w] = Mnew[2 * w];
    M0[2 * w + 1] = Mnew[2 * w + 1];
}

__global__ void thermal_cweight_kernel(double *weight, cplx *M0, const cplx *Mnew, const cplx *cmf, const cplx *cfb, int nw) {
    thc_weight_update<false>(weight, M0, Mnew, cmf, cfb, cmake(1.0, 0.0), nw);
}

__global__ void thermal_cweight_mf_kernel(double *weight, cplx *M0, const cplx *Mnew, const cplx *cmf, const cplx *cfb,
                                          cplx mfc, int nw) {
    thc_weight_update<true>(weight, M0, Mnew, cmf, cfb, mfc, nw);
}

// ---- a dense real trial and a dense real BH1 with a diagonal field exponential: the Hubbard model with continuous
// fields (thermal_propagation/continuous.py:84-120,202-257, hubbard.py:199-250, stack.py:299-324, non-diagonal branch).

// LDS of thermal_cslice_dense_kernel: B and the new right (complex), bv[64], and BH1_s (real), all of pitch M | 1.
// BH1_s is the operand of both products that make B_s and is read M / 16 times per tile: it is staged once per spin.
// right (read once, as the B operand of one product) and left_k (read once, as the A operand of the last) stay in
// device memory.
inline size_t thd_slice_lds(int M) { return sizeof(cplx) * (2 * ts_mat(M) + 64) + sizeof(double) * ts_mat(M); }

// PropagatorStack.set_all and update_full_rank, non-diagonal branch (stack.py:238-243,309-310), on the host: BTpow
// [2, M, M] = BT left-multiplied stack_size times onto I, left [stack_size, 2, M, M] with left_k = left_(k - 1) BT_inv,
// left_(-1) = BTpow.  Every element of a product is one chain of fused multiply-adds over k in ascending order from 0,
// which is how the reference's matrix product (dgemm at these sizes) rounds.
inline void thd_left_table(int M, int stack_size, const double *BT, const double *BT_inv, double *BTpow, double *left) {
    const size_t mm = (size_t)M * M;
    std::vector<double> tmp(mm);
    auto matmul = [&](const double *A, const double *B, double *C) {     // C = A B
        for (int i = 0; i < M; ++i)
            for (int j = 0; j < M; ++j) {
                double acc = 0.0;
                for (int k = 0; k < M; ++k) acc = std::fma(A[(size_t)i * M + k], B[(size_t)k * M + j], acc);
                C[(size_t)i * M + j] = acc;
            }
    };
    for (int s = 0; s < 2; ++s) {
        double *p = BTpow + s * mm;
        for (size_t e = 0; e < mm; ++e) p[e] = 0.0;
        for (int i = 0; i < M; ++i) p[(size_t)i * M + i] = 1.0;
        for (int it = 0; it < stack_size; ++it) {
            matmul(BT + s * mm, p, tmp.data());
            memcpy(p, tmp.data(), sizeof(double) * mm);
        }
        const double *prev = p;
        for (int k = 0; k < stack_size; ++k) {
            double *lk = left + ((size_t)k * 2 + s) * mm;
            matmul(prev, BT_inv + s * mm, lk);
            prev = lk;
        }
    }
}

struct ThdSliceArgs {
    const cplx *bv;             // [nw, M] diagonal of BV
    cplx *right, *stack;        // [nw, 2, M, M], [nw, nbins, 2, M, M]
    const double *bh1, *left;   // [2, M, M]: BH1, and left_k of the slice being added
    int M, nbins, block, counter;
};

// C = A B with A real and B complex, as ts_gemm: two real MFMA products per step where the complex form takes four
template <class LA, class LB, class ST>
__device__ inline void thd_gemm_rc(int M, LA la, LB lb, ST st) {
    typedef TsScalar<cplx> S;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const int nt = (M + 15) >> 4, lr = lane & 15, lk = lane >> 4;
    for (int tile = wave; tile < nt * nt; tile += nwave) {
        const int row0 = (tile / nt) << 4, col0 = (tile % nt) << 4;
        const int arow = row0 + lr, bcol = col0 + lr;
        S::Acc acc = S::acc0();
        for (int k0 = 0; k0 < M; k0 += 4) {
            const int k = k0 + lk;
            const double a = (arow < M && k < M) ? la(arow, k) : 0.0;
            const cplx b = (bcol < M && k < M) ? lb(k, bcol) : S::zero();
            acc.re = mfma16(a, b.x, acc.re);
            acc.im = mfma16(a, b.y, acc.im);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + lk + 4 * r;
            if (row < M && bcol < M) st(row, bcol, S::at(acc, r));
        }
    }
}

// LDS of the slice kernel with one staging matrix (AFQ_THERMAL_WIDE): the matrix and bv[128]
inline size_t thd_slice_wide_lds(int M) { return sizeof(cplx) * (ts_mat(M) + TW_COLS); }

// (no matrix in LDS, AFQ_THERMAL_FAR: thd_slice_far_lds of thermal_wide.h -- bv[128] alone)
// An operand of the next product where the product can read it.  THC_IN_LDS and THC_NONE_IN_LDS: where it is (LDS, or
// the walker's scratch).  THC_ONE_IN_LDS: it is copied from the walker's scratch into the one staging matrix Z in LDS,
// behind a barrier.  `also`, where given, gets a copy in device memory on the way (pitch M).
template <ThcPlace P> __device__ inline TsMatView<cplx> thd_staged(TsMatView<cplx> src, cplx *Z, cplx *also, int M) {
    constexpr bool STAGE = P == THC_ONE_IN_LDS;
    if (!STAGE && !also) return src;
    const int LD = M | 1;
    for (int e = threadIdx.x; e < M * M; e += TH_THREADS) {
        const int r = e / M, c = e % M;
        const cplx x = src(r, c);
        if (also) also[e] = x;
        if (STAGE) Z[r * LD + c] = x;
    }
    if (!STAGE) return src;
    __syncthreads();
    return {Z, LD};
}

// One work-group per walker.  Per spin: B = BH1 (BV BH1) with the diagonal BV folded into the loader of the product's
// complex operand; right <- B right (right = B at in-bin counter 0); bin[block] = left_k right.
// IN_LDS: B and the new right are two complex matrices in LDS, beside bv[64] and BH1_s (real).  Otherwise (the wide
// route) one staging matrix in LDS holds in turn BH1_s, B_s (the A operand of right <- B right) and the new right (the B
// operand of left_k right); B_s and the new right pass through two [M, M] buffers of the walker's scratch in device
// memory (scratch + w stride, pitch M).  THC_NONE_IN_LDS (the far route): B_s and the new right in scratch as well, and
// every operand read where it lies: BH1_s in a.bh1, B_s and the new right in scratch; LDS holds bv alone.  The products
// are the same with other loaders: the same bits where they run.
// bv holds M entries of the dynamic LDS the launch gives: thd_slice_far_lds (128 entries) on the far route, and the same
// THC_NONE_IN_LDS instantiation with thd_slice_quad_lds (256 entries) under the quad route's name.  It is filled by the
// threads tid < M, so M <= TH_THREADS.
template <ThcPlace P> __global__ __launch_bounds__(TH_THREADS) void thermal_cslice_dense_kernel(ThdSliceArgs a, cplx *scratch, long stride) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr bool IN_LDS = P == THC_IN_LDS, FAR = P == THC_NONE_IN_LDS;
    const int M = a.M, LD = M | 1, tid = threadIdx.x, w = blockIdx.x;
    const size_t mat = ts_mat(M);
    const long mm = (long)M * M;
    cplx *Z = (cplx *)smem, *bv = Z + (IN_LDS ? 2 : FAR ? 0 : 1) * mat;
    double *H = IN_LDS ? (double *)(bv + 64) : (double *)Z;
    TsMatView<cplx> B = {Z, LD}, T2 = {Z + mat, LD};
    if (!IN_LDS) { B = {scratch + (long)w * stride, M}; T2 = {B.p + mm, M}; }
    if (tid < M) bv[tid] = a.bv[(long)w * M + tid];
    for (int s = 0; s < 2; ++s) {
        const double *Hs = a.bh1 + s * mm, *lf = a.left + s * mm;
        cplx *R = a.right + ((long)w * 2 + s) * mm;
        cplx *S = a.stack + (((long)w * a.nbins + a.block) * 2 + s) * mm;
        if (!FAR) for (int e = tid; e < M * M; e += TH_THREADS) H[(e / M) * LD + e % M] = Hs[e];
        __syncthreads();
        const auto bh = [&](int r, int k) { return FAR ? Hs[r * M + k] : H[r * LD + k]; };
        thd_gemm_rc(M, bh, [&](int k, int c) { return cscale(bv[k], bh(k, c)); }, [&](int r, int c, cplx x) { B(r, c) = x; });
        __syncthreads();
        TsMatView<cplx> Rn = B;
        if (a.counter != 0) {
            const TsMatView<cplx> Bs = thd_staged<P>(B, Z, nullptr, M);
            ts_gemm<cplx>(M, [&](int r, int k) { return Bs(r, k); }, [&](int k, int c) { return R[k * M + c]; },
                          [&](int r, int c, cplx x) { T2(r, c) = x; });
            __syncthreads();
            Rn = T2;
        }
        const TsMatView<cplx> Rs = thd_staged<P>(Rn, Z, R, M);
        thd_gemm_rc(M, [&](int r, int k) { return lf[r * M + k]; }, [&](int k, int c) { return Rs(k, c); },
                    [&](int r, int c, cplx x) { S[r * M + c] = x; });
        __syncthreads();
    }
}

// continuous.py:97-115 with hubbard.py:241-250 for one walker per work-group: vbias_i = i sqrt(U) (P_up,ii + P_dn,ii)
// from the diagonal of P [nw, 2, M, M], xbar = -sqrt(dt) (vbias - mf) clipped at 1, xs, cmf, cfb as
// thermal_cfields_kernel makes them, and the diagonal of BV: bv_i = sum_{n <= 6} v^n / n!, v = sqrt(dt) i sqrt(U) xs_i,
// by the reference's recurrence t <- v t / n.
__global__ __launch_bounds__(TH_THREADS) void thermal_cfields_dense_kernel(const cplx *P, const double *xi, const cplx *mf,
                                                                             cplx *xbar, cplx *xs, cplx *cmf, cplx *cfb,
                                                                             cplx *bv, int M, double sqrt_dt, double sqrt_u,
                                                                             unsigned long long *counters) {
    const int w = blockIdx.x, tid = threadIdx.x;
    const long mm = (long)M * M;
    const cplx *Pw = P + (long)w * 2 * mm;
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int n = tid; n < M; n += TH_THREADS) {
        const long e = (long)w * M + n;
        const cplx pu = Pw[(long)n * M + n], pd = Pw[mm + (long)n * M + n], m = mf[n];
        const cplx v = cmake(-sqrt_u * (pu.y + pd.y), sqrt_u * (pu.x + pd.x));
        const cplx sft = thc_field_terms(cmake(-sqrt_dt * (v.x - m.x), -sqrt_dt * (v.y - m.y)), 1.0, xi[e], m, e, xbar, xs, acc);
        const double f = sqrt_dt * sqrt_u;
        const cplx vh = cmake(-f * sft.y, f * sft.x);
        cplx t = cmake(1.0, 0.0), phi = cmake(1.0, 0.0);
        for (int q = 1; q <= 6; ++q) {
            t = cmul(vh, t);
            t = cmake(t.x / (double)q, t.y / (double)q);
            phi = cadd(phi, t);
        }
        bv[e] = phi;
    }
    thc_field_sums(acc, w, sqrt_dt, cmf, cfb, counters);
}

// walker blockIdx.y: bins <- diag(BTpow) [2, M], or with dense the matrices BTpow [2, M, M]; unless bins_only also
// G <- G0, right <- I, weight <- 1, and with_m0 M0 <- M00
__global__ void thermal_creset_kernel(cplx *stack, cplx *G, cplx *right, cplx *M0, double *weight, const double *BTpow,
                                      const cplx *G0, const cplx *M00, int nbins, int M, int bins_only, int with_m0,
                                      int dense) {
    const long per = 2L * M * M;
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const int w = blockIdx.y;
    if (i < per) {
        const int s = (int)(i / ((long)M * M)), r = (int)((i / M) % M), c = (int)(i % M);
        const cplx b = cmake(dense ? BTpow[i] : r == c ? BTpow[s * M + r] : 0.0, 0.0);
        for (int n = 0; n < nbins; ++n) stack[((long)w * nbins + n) * per + i] = b;
        if (!bins_only) {
            G[(long)w * per + i] = G0[i];
            right[(long)w * per + i] = cmake(r == c ? 1.0 : 0.0, 0.0);
        }
    }
    if (bins_only) return;
    if (with_m0 && i < 2) M0[2 * w + i] = M00[i];
    if (i == 0) weight[w] = 1.0;
}

}  // namespace

int k_thermal_c_greens(afq_handle *h, int slice_ix) {
    return th_launch_greens<cplx>(h, h->thc_stack, h->thc_G, h->thc_det, ts_first_bin(h, slice_ix), -1, dim3(2 * h->nw));
}

// walkers/handler.py:424-430: bins, G, weight.  The reference's reset leaves walker.M0 at the determinant the last path
// ended with, and the first slice of the next path divides by it: with_m0 (a fresh population) puts the trial's there.
int k_thermal_c_reset(afq_handle *h, bool with_m0) {
    const int M = h->M, nbins = h->th_nbins;
    const long per = 2L * M * M;
    // the trial's G and M0 once, from walker 0's fresh bins (every bin is BT^stack_size), then broadcast
    const int dense = h->th_kind == TH_CPLX_DENSE ? 1 : 0;
    AFQ_LAUNCH(h, thermal_creset_kernel, dim3((unsigned)((per + 255) / 256), 1), dim3(256), 0, h->stream, h->thc_stack, h->thc_G,
               h->thc_right, h->thc_M0, h->weight, h->thc_BTpow, h->thc_G0, h->thc_M00, nbins, M, 1, 0, dense);
    AFQ_POST(h);
    AFQ_TRY(th_launch_greens<cplx>(h, h->thc_stack, h->thc_G0, h->thc_M00, ts_first_bin(h, 0), 0, dim3(2)));
    AFQ_LAUNCH(h, thermal_creset_kernel, dim3((unsigned)((per + 255) / 256), h->nw), dim3(256), 0, h->stream, h->thc_stack,
               h->thc_G, h->thc_right, h->thc_M0, h->weight, h->thc_BTpow, h->thc_G0, h->thc_M00, nbins, M, 0, with_m0 ? 1 : 0, dense);
    AFQ_POST(h);
    h->th_slice = 0; h->th_block = 0; h->th_counter = 0;
    return AFQ_OK;
}

int k_thermal_c_sweep_greens(afq_handle *h, cplx *Gs, cplx *Ts, int ts0, int nb) {
    return th_launch_greens<cplx>(h, h->thc_stack, h->thc_G, h->thc_det, 0, -1, dim3(2 * h->nw, nb), Gs, Ts, ts0);
}

int k_thermal_c_sweep_rdm(afq_handle *h, const cplx *Gs, cplx *P, double *nav, int n) { return ts_launch_rdm_n<cplx>(h, Gs, P, nav, n); }

int k_thermal_c_energy(afq_handle *h, double *E_out, double *nav_out) {
    AFQ_TRY(ts_launch_rdm<cplx>(h, h->thc_G, h->th_nav));
    if (h->th_kind == TH_CPLX_DENSE) {                  // Hubbard: the full-G energy of P, as the real walkers' (k_thermal.hip)
        AFQ_TRY(k_energy_hubbard_full_g(h, h->G, h->nw, h->energy));
        return th_energy_out(h, E_out, nav_out);
    }
    cplx *two = nullptr, *E = nullptr;                  // (the per-q pair sums are scratch here)
    AFQ_TRY(k_ueg_sf_two(h, h->nw, &two, &E));
    AFQ_TRY(k_ueg_pair_sums(h, h->G, h->nw, h->energy, two));
    return th_energy_out(h, E_out, nav_out);
}

namespace {

// ---- configuring: what the two entry points share

const char *const THC_RESIDENT_HINT = "; AFQ_THERMAL_STREAMED_GREENS (streamed_greens) keeps T in device memory and reaches further";

// STREAMED_GREENS, WIDE, FAR and QUAD name four placements of the same working set: any two together mean nothing
int thc_engine_of(afq_handle *h, const std::string &me, int options, ThEngine *engine) {
    const bool streamed = (options & AFQ_THERMAL_STREAMED_GREENS) != 0, wide = (options & AFQ_THERMAL_WIDE) != 0,
               far = (options & AFQ_THERMAL_FAR) != 0, quad = (options & AFQ_THERMAL_QUAD) != 0;
    if (streamed && wide)
        AFQ_FAIL(h, AFQ_EINVAL, me + "wide_basis and streamed_greens are two placements of the same matrices: ask for one");
    if (far && wide)
        AFQ_FAIL(h, AFQ_EINVAL, me + "far_basis and wide_basis are two placements of the same matrices: ask for one");
    if (far && streamed)
        AFQ_FAIL(h, AFQ_EINVAL, me + "far_basis and streamed_greens are two placements of the same matrices: ask for one");
    if (quad && far)
        AFQ_FAIL(h, AFQ_EINVAL, me + "quad_basis and far_basis are two placements of the same matrices: ask for one");
    if (quad && wide)
        AFQ_FAIL(h, AFQ_EINVAL, me + "quad_basis and wide_basis are two placements of the same matrices: ask for one");
    if (quad && streamed)
        AFQ_FAIL(h, AFQ_EINVAL, me + "quad_basis and streamed_greens are two placements of the same matrices: ask for one");
    *engine = quad ? TH_ENGINE_QUAD : far ? TH_ENGINE_FAR : wide ? TH_ENGINE_WIDE : streamed ? TH_ENGINE_STREAMED : TH_ENGINE_RESIDENT;
    return AFQ_OK;
}

const ThLds THC_WIDE_GREENS = {"the wide Green's function (thermal_cgreens_wide_kernel)", ts_greens_wide_lds<cplx>, ""};

// two columns per lane: the wide route and the far route
inline bool thc_two_columns(ThEngine engine) { return engine == TH_ENGINE_WIDE || engine == TH_ENGINE_FAR; }
// scalars of th_scratch per work-group of the handle's Green's kernel; a walker's share is both spins'
inline size_t thc_greens_scratch(ThEngine engine, int M) {
    return engine == TH_ENGINE_FAR || engine == TH_ENGINE_QUAD ? ts_greens_far_scratch(M) : engine == TH_ENGINE_WIDE ? ts_greens_wide_scratch(M)
         : engine == TH_ENGINE_STREAMED ? TsStreamed<cplx>::scratch(M) : (size_t)0;
}

// th_screen_bound in the words of the continuous fields: the kernels first, then lane = column (wide: two columns per
// lane, quad: four).  who: "" or ", Hubbard"; unit: what M counts.
int thc_screen_bound(afq_handle *h, const char *who, const char *unit, ThEngine engine, std::initializer_list<ThLds> need) {
    return th_screen_bound(h, std::string("thermal walkers with continuous fields") + who +
                           (engine == TH_ENGINE_STREAMED ? " (streamed_greens)" : engine == TH_ENGINE_WIDE ? " (wide_basis)"
                            : engine == TH_ENGINE_FAR ? " (far_basis)" : engine == TH_ENGINE_QUAD ? " (quad_basis)" : ""),
                           unit, engine == TH_ENGINE_QUAD ? TQ_COLS : thc_two_columns(engine) ? TW_COLS : THC_LANES, false, need);
}

// Behind an entry point's own checks: its host-built tables (`per` numbers per slice: 2 M diagonals or 2 M M), the
// walkers' buffers, the path's shape, the kind, and a fresh population.
int thc_configure_common(afq_handle *h, ThKind kind, int ntime_slices, int stack_size, double dt, ThEngine engine, double fb_bound,
                         const double *BTpow, const double *left, const double *bh1, size_t per, const double *mf_shift) {
    const size_t mm = (size_t)h->M * h->M, n = h->nw;
    const int nbins = ntime_slices / stack_size;
    int rc;
    if ((rc = dev_upload(h, LT_WALKERS, &h->thc_BTpow, BTpow, per)) ||
        (rc = dev_upload(h, LT_WALKERS, &h->thc_left, left, (size_t)stack_size * per)) ||
        (rc = dev_upload(h, LT_WALKERS, &h->thc_bh1, bh1, per)) ||
        (rc = dev_upload(h, LT_WALKERS, &h->thc_mf, mf_shift, (size_t)h->K))) return rc;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->thc_G, 2 * mm * n)) || (rc = dev_alloc(h, LT_WALKERS, &h->thc_G0, 2 * mm)) ||
        (rc = dev_alloc(h, LT_WALKERS, &h->thc_stack, 2 * mm * n * nbins)) || (rc = dev_alloc(h, LT_WALKERS, &h->thc_right, 2 * mm * n)) ||
        (rc = dev_alloc(h, LT_WALKERS, &h->thc_M0, 2 * n)) || (rc = dev_alloc(h, LT_WALKERS, &h->thc_M00, (size_t)2)) ||
        (rc = dev_alloc(h, LT_WALKERS, &h->thc_det, 2 * n)) || (rc = dev_alloc(h, LT_WALKERS, &h->th_nav, n))) return rc;
    // T of the streamed Green's kernel, two buffers per (walker, spin); the wide route's scratch, four per (walker,
    // spin), of which the wide slice kernels use the walker's first two; the far and the quad route's, W behind the
    // four (nw 2 (4 M M + M (M | 1)) scalars, in size_t: 2.7 GB at M = 256 and 256 walkers); a handle configured
    // without any of them holds none
    const size_t scratch = 2 * thc_greens_scratch(engine, h->M) * n;
    if ((rc = dev_alloc(h, LT_WALKERS, (cplx **)&h->th_scratch, scratch))) return rc;
    h->th_engine = engine;
    if ((rc = ensure_G(h))) return rc;                  // c128 [nw, 2, M, M]: the one-body density matrices
    h->thc_fb_bound = fb_bound;
    h->dt = dt; h->sqrt_dt = std::pow(dt, 0.5);        // (the handle's time step, as afq_set_propagator sets it)
    h->th_L = ntime_slices; h->th_ss = stack_size; h->th_nbins = nbins; h->th_nstblz = 1;
    h->th_kind = kind;
    return k_thermal_c_reset(h, true);
}

// ---- one slice: the two steps that depend on the trial's kind

// UEG: vbias = P . [iA | iB], xbar = -sqrt(dt) vbias clipped at fb_bound, xs, cmf, cfb (planewave.py:219-276), VHS,
// and the slice kernel on the trial's diagonals
int thc_slice_diag(afq_handle *h) {
    const int M = h->M;
    AFQ_TRY(k_vbias_ueg(h));
    AFQ_LAUNCH(h, thermal_cfields_kernel, dim3(h->nw), dim3(TH_THREADS), 0, h->stream, h->vbias, h->xi, h->thc_mf, h->xbar,
               h->xs, h->cmf, h->cfb, h->K, h->sqrt_dt, h->thc_fb_bound, h->counters);
    AFQ_POST(h);
    AFQ_TRY(k_vhs_ueg(h));                              // VHS = sqrt(dt) (iA xs[:nq] + iB xs[nq:])
    ThcSliceArgs a;
    a.vhs = h->vhs; a.right = h->thc_right; a.stack = h->thc_stack; a.bh1 = h->thc_bh1;
    a.left = h->thc_left + (size_t)h->th_counter * 2 * M;
    a.M = M; a.nbins = h->th_nbins; a.block = h->th_block; a.counter = h->th_counter;
    cplx *const scratch = (cplx *)h->th_scratch;
    const long stride = (long)(2 * thc_greens_scratch(h->th_engine, M));     // a walker's: both spins' of the Green's kernel
    if (h->th_engine == TH_ENGINE_QUAD)
        return th_launch<thermal_cslice_kernel<THC_NONE_IN_LDS>>(h, "thermal_cslice_quad_kernel", dim3(h->nw), thc_slice_quad_lds(M), a, scratch, stride);
    if (h->th_engine == TH_ENGINE_FAR)
        return th_launch<thermal_cslice_kernel<THC_NONE_IN_LDS>>(h, "thermal_cslice_far_kernel", dim3(h->nw), thc_slice_far_lds(M), a, scratch, stride);
    if (h->th_engine == TH_ENGINE_WIDE)
        return th_launch<thermal_cslice_kernel<THC_ONE_IN_LDS>>(h, "thermal_cslice_wide_kernel", dim3(h->nw), thc_slice_wide_lds(M), a, scratch, stride);
    return th_launch<thermal_cslice_kernel<THC_IN_LDS>>(h, "thermal_cslice_kernel", dim3(h->nw), thc_slice_lds(M), a, scratch, stride);
}

// Hubbard: the force bias, the clip at 1, xs, cmf, cfb and the diagonal of BV from P's diagonal, and the slice kernel
// on the trial's matrices
int thc_slice_dense(afq_handle *h) {
    const int M = h->M;
    AFQ_LAUNCH(h, thermal_cfields_dense_kernel, dim3(h->nw), dim3(TH_THREADS), 0, h->stream, h->G, h->xi, h->thc_mf,
               h->xbar, h->xs, h->cmf, h->cfb, h->vhs, M, h->sqrt_dt, h->thd_sqrt_u, h->counters);
    AFQ_POST(h);
    ThdSliceArgs a;
    a.bv = h->vhs; a.right = h->thc_right; a.stack = h->thc_stack; a.bh1 = h->thc_bh1;
    a.left = h->thc_left + (size_t)h->th_counter * 2 * M * M;
    a.M = M; a.nbins = h->th_nbins; a.block = h->th_block; a.counter = h->th_counter;
    cplx *const scratch = (cplx *)h->th_scratch;
    const long stride = (long)(2 * thc_greens_scratch(h->th_engine, M));     // a walker's: both spins' of the Green's kernel
    if (h->th_engine == TH_ENGINE_QUAD)
        return th_launch<thermal_cslice_dense_kernel<THC_NONE_IN_LDS>>(h, "thermal_cslice_dense_quad_kernel", dim3(h->nw), thd_slice_quad_lds(M), a,
                                                                                scratch, stride);
    if (h->th_engine == TH_ENGINE_FAR)
        return th_launch<thermal_cslice_dense_kernel<THC_NONE_IN_LDS>>(h, "thermal_cslice_dense_far_kernel", dim3(h->nw), thd_slice_far_lds(M), a,
                                                                       scratch, stride);
    if (h->th_engine == TH_ENGINE_WIDE)
        return th_launch<thermal_cslice_dense_kernel<THC_ONE_IN_LDS>>(h, "thermal_cslice_dense_wide_kernel", dim3(h->nw), thd_slice_wide_lds(M), a,
                                                                      scratch, stride);
    return th_launch<thermal_cslice_dense_kernel<THC_IN_LDS>>(h, "thermal_cslice_dense_kernel", dim3(h->nw), thd_slice_lds(M), a, scratch, stride);
}

// the phaseless weight from the determinant ratio; the dense kind's carries the constant of the mean-field shift
int thc_weight(afq_handle *h) {
    if (h->th_kind == TH_CPLX_DENSE)
        AFQ_LAUNCH(h, thermal_cweight_mf_kernel, dim3((h->nw + 127) / 128), dim3(128), 0, h->stream, h->weight, h->thc_M0,
                   h->thc_det, h->cmf, h->cfb, cmake(h->thd_mf_const[0], h->thd_mf_const[1]), h->nw);
    else
        AFQ_LAUNCH(h, thermal_cweight_kernel, dim3((h->nw + 127) / 128), dim3(128), 0, h->stream, h->weight, h->thc_M0, h->thc_det,
                   h->cmf, h->cfb, h->nw);
    AFQ_POST(h);
    return AFQ_OK;
}

}  // namespace

extern "C" {

int afq_thermal_configure_continuous(afq_handle *h, int ntime_slices, int stack_size, double dt, const double *BT,
                                     const double *BT_inv, const double *BH1, const double *mf_shift, double fb_bound,
                                     int options) {
    AFQ_API(h, "afq_thermal_configure_continuous");
    if (!h) return AFQ_EINVAL;
    h->th_kind = TH_NONE;
    const ThEntry me = {"afq_thermal_configure_continuous: ", AFQ_THERMAL_STREAMED_GREENS | AFQ_THERMAL_WIDE | AFQ_THERMAL_FAR | AFQ_THERMAL_QUAD, AFQ_EINVAL,
                        "afq_thermal_configure_continuous: charge_decomposition belongs to the discrete fields", AFQ_SYS_UEG,
                        "thermal walkers with continuous fields: UEG systems only (no Generic, no continuous Hubbard)", "both"};
    if (!BT || !BT_inv || !BH1 || !mf_shift) AFQ_FAIL(h, AFQ_EINVAL, me.me + "null operand");
    AFQ_TRY(th_screen_options(h, me, options));
    ThEngine route;
    AFQ_TRY(thc_engine_of(h, me.me, options, &route));
    const ThLds slice = {"the slice kernel (thermal_cslice_kernel)", thc_slice_lds, ""};
    if (route == TH_ENGINE_QUAD)
        AFQ_TRY(thc_screen_bound(h, "", "plane waves", route, {THC_QUAD_GREENS, THC_QUAD_SLICE}));
    else if (route == TH_ENGINE_FAR)
        AFQ_TRY(thc_screen_bound(h, "", "plane waves", route, {THC_FAR_GREENS, THC_FAR_SLICE}));
    else if (route == TH_ENGINE_WIDE)
        AFQ_TRY(thc_screen_bound(h, "", "plane waves", route, {THC_WIDE_GREENS,
                {"the wide slice kernel (thermal_cslice_wide_kernel)", thc_slice_wide_lds, ""}}));
    else if (route == TH_ENGINE_STREAMED)
        AFQ_TRY(thc_screen_bound(h, "", "plane waves", route, {slice,
                {"the streamed Green's function (thermal_cgreens_streamed_kernel)", ts_greens_streamed_lds<cplx>, ""}}));
    else
        AFQ_TRY(thc_screen_bound(h, "", "plane waves", route, {{"the complex Green's function", ts_greens_lds<cplx>, THC_RESIDENT_HINT}, slice}));
    AFQ_TRY(th_screen_state(h, me, ntime_slices, stack_size, 1));
    if (!(dt > 0.0) || !(fb_bound >= 0.0)) AFQ_FAIL(h, AFQ_EINVAL, me.me + "dt must be positive, fb_bound not negative");
    const int M = h->M;
    const size_t mm = (size_t)M * M;
    for (int s = 0; s < 2; ++s)
        for (int i = 0; i < M; ++i)
            for (int j = 0; j < M; ++j)
                if (i != j && (BT[s * mm + (size_t)i * M + j] != 0.0 || BT_inv[s * mm + (size_t)i * M + j] != 0.0))
                    AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers with continuous fields: a diagonal trial density matrix only (OneBody on plane waves)");
    hipSetDevice(h->device);
    // PropagatorStack.set_all and update_full_rank with a diagonal trial (stack.py:229-236,305-307): left = BT applied
    // stack_size times to 1; the k-th slice of a bin multiplies it by BT_inv once more.  The reference reads only the
    // diagonal of BH1 (planewave.py:462-469).
    std::vector<double> pw(2 * (size_t)M, 1.0), left((size_t)stack_size * 2 * M), bh(2 * (size_t)M);
    for (int s = 0; s < 2; ++s)
        for (int i = 0; i < M; ++i) {
            const double b = BT[s * mm + (size_t)i * M + i], bi = BT_inv[s * mm + (size_t)i * M + i];
            double p = 1.0;
            for (int it = 0; it < stack_size; ++it) p = b * p;
            pw[(size_t)s * M + i] = p;
            for (int k = 0; k < stack_size; ++k) { p = p * bi; left[((size_t)k * 2 + s) * M + i] = p; }
            bh[(size_t)s * M + i] = BH1[s * mm + (size_t)i * M + i];
        }
    return thc_configure_common(h, TH_CPLX_DIAG, ntime_slices, stack_size, dt, route, fb_bound, pw.data(), left.data(),
                                bh.data(), 2 * (size_t)M, mf_shift);
}

int afq_thermal_wide_max_basis(void) {
    int m = TW_COLS;
    while (m > 1 && (ts_greens_wide_lds<cplx>(m) > TH_LDS_MAX || thc_slice_wide_lds(m) > TH_LDS_MAX || thd_slice_wide_lds(m) > TH_LDS_MAX)) --m;
    return m;
}

int afq_thermal_far_max_basis(void) { return th_far_bound(); }

int afq_thermal_quad_max_basis(void) { return th_quad_bound(); }

int afq_thermal_left_table(int M, int stack_size, const double *BT, const double *BT_inv, double *BTpow_out, double *left_out) {
    if (M < 1 || stack_size < 1 || !BT || !BT_inv || !BTpow_out || !left_out) return AFQ_EINVAL;
    thd_left_table(M, stack_size, BT, BT_inv, BTpow_out, left_out);
    return AFQ_OK;
}

int afq_thermal_configure_hubbard_continuous(afq_handle *h, int ntime_slices, int stack_size, double dt, const double *BT,
                                             const double *BT_inv, const double *BH1, const double *mf_shift,
                                             const double *mf_const_fac, int options) {
    AFQ_API(h, "afq_thermal_configure_hubbard_continuous");
    if (!h) return AFQ_EINVAL;
    h->th_kind = TH_NONE;
    const ThEntry me = {"afq_thermal_configure_hubbard_continuous: ", AFQ_THERMAL_STREAMED_GREENS | AFQ_THERMAL_WIDE | AFQ_THERMAL_FAR | AFQ_THERMAL_QUAD, AFQ_EINVAL,
                        "afq_thermal_configure_hubbard_continuous: charge_decomposition belongs to the discrete fields (the "
                        "continuous form is the charge form alone)", AFQ_SYS_HUBBARD,
                        "thermal walkers with continuous fields and a dense trial: Hubbard systems only (no Generic)", "both"};
    if (!BT || !BT_inv || !BH1 || !mf_shift || !mf_const_fac) AFQ_FAIL(h, AFQ_EINVAL, me.me + "null operand");
    AFQ_TRY(th_screen_options(h, me, options));
    ThEngine route;
    AFQ_TRY(thc_engine_of(h, me.me, options, &route));
    const bool streamed = route == TH_ENGINE_STREAMED;
    const ThLds greens = route == TH_ENGINE_QUAD ? THC_QUAD_GREENS : route == TH_ENGINE_FAR ? THC_FAR_GREENS : route == TH_ENGINE_WIDE ? THC_WIDE_GREENS : streamed ? ThLds{"the streamed Green's function (thermal_cgreens_streamed_kernel)", ts_greens_streamed_lds<cplx>, ""}
                                   : ThLds{"the complex Green's function (thermal_cgreens_kernel)", ts_greens_lds<cplx>, THC_RESIDENT_HINT};
    const ThLds slice = route == TH_ENGINE_QUAD ? THD_QUAD_SLICE : route == TH_ENGINE_FAR ? THD_FAR_SLICE : route == TH_ENGINE_WIDE ? ThLds{"the wide slice kernel (thermal_cslice_dense_wide_kernel)", thd_slice_wide_lds, ""}
                                                : ThLds{"the slice kernel (thermal_cslice_dense_kernel)", thd_slice_lds, ""};
    AFQ_TRY(thc_screen_bound(h, ", Hubbard", "sites", route, {greens, slice}));
    AFQ_TRY(th_screen_state(h, me, ntime_slices, stack_size, 1));
    if (!(dt > 0.0)) AFQ_FAIL(h, AFQ_EINVAL, me.me + "dt must be positive");
    if (!(h->U >= 0.0)) AFQ_FAIL(h, AFQ_EINVAL, me.me + "U must not be negative (iu_fac = i sqrt(U))");
    hipSetDevice(h->device);
    const size_t mm = (size_t)h->M * h->M;
    std::vector<double> pw(2 * mm), left((size_t)stack_size * 2 * mm);
    thd_left_table(h->M, stack_size, BT, BT_inv, pw.data(), left.data());
    h->thd_mf_const[0] = mf_const_fac[0]; h->thd_mf_const[1] = mf_const_fac[1];
    h->thd_sqrt_u = std::pow(h->U, 0.5);
    return thc_configure_common(h, TH_CPLX_DENSE, ntime_slices, stack_size, dt, route, 1.0, pw.data(), left.data(), BH1,
                                2 * mm, mf_shift);
}

int afq_thermal_propagate_continuous(afq_handle *h, const double *xi, double *xi_out) {
    AFQ_API(h, "afq_thermal_propagate_continuous");
    if (!h) return AFQ_EINVAL;
    AFQ_TRY(th_need(h, true));
    if (h->th_slice >= h->th_L) AFQ_FAIL(h, AFQ_ESTATE, "afq_thermal_propagate_continuous: the path is complete (afq_thermal_reset starts the next)");
    const size_t nf = (size_t)h->nw * h->K;
    // the fields of every walker, dead ones included (the thermal driver skips none): the host's, or the device stream
    if (xi) AFQ_HIP(h, hipMemcpyAsync(h->xi, xi, sizeof(double) * nf, hipMemcpyHostToDevice, h->stream));
    else AFQ_TRY(k_rng_normal_into(h, h->xi, (long)nf));
    AFQ_TRY(ts_launch_rdm<cplx>(h, h->thc_G, nullptr));                // P = I - G^T
    AFQ_TRY(h->th_kind == TH_CPLX_DENSE ? thc_slice_dense(h) : thc_slice_diag(h));
    th_advance(h);
    // G = [I + S_{nbins - 1} .. S_0]^-1 on the walker's current bins, Mnew = det G, the weight
    AFQ_TRY(th_launch_greens<cplx>(h, h->thc_stack, h->thc_G, h->thc_det, 0, -1, dim3(2 * h->nw)));
    AFQ_TRY(thc_weight(h));
    if (xi_out) return copy_out(h, xi_out, h->xi, sizeof(double) * nf);
    return AFQ_OK;
}

}  // extern "C"
