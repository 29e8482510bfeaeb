// Finite-temperature AFQMC walkers with continuous Hubbard-Stratonovich fields for the uniform electron gas
// (thermal_propagation/planewave.py:219-276,445-517, walkers/stack.py:299-324, walkers/thermal.py:51-64,472-547 of the
// reference; phaseless path, force bias on, full-rank walkers, diagonal one-body trial density matrix).  Every matrix of
// the walker is complex: G_s c128 [2, M, M], the bins c128 [nbins, 2, M, M], the running product of the current bin
// `right` c128 [2, M, M] and M0_s = det G_s c128 [2].  The slice counter, the block and the in-bin counter are the
// handle's, as for the real walkers of k_thermal.hip.  A walker's working set stays in LDS: 4 complex matrices of pitch
// M | 1, which the 160 KiB of a compute unit hold up to M = 47 (the plane-wave shells: 7, 19, 27, 33; 57 does not fit).
// With AFQ_THERMAL_STREAMED_GREENS the Green's function keeps 2 matrices in LDS and T in the handle's thc_tscratch; the
// bound is then the slice kernel's three matrices: M = 57, the next shell.  81 is refused either way.
//
//   thermal_cgreens_kernel  G and det G of every (walker, spin) from the stack: thermal_strat.h's engine with T = cplx.
//   thermal_cgreens_streamed_kernel  the same from thermal_strat.h's streamed form, for a handle configured with the bit.
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
#include <cstring>

#define THC_LDS_MAX (160 * 1024)
#define THC_LANES 64            // the engine works lane = column

namespace {

inline size_t thc_slice_lds(int M) { return sizeof(cplx) * 3 * ts_mat(M); }

struct ThcSliceArgs {
    const cplx *vhs;            // [nw, M, M]
    cplx *right, *stack;        // [nw, 2, M, M], [nw, nbins, 2, M, M]
    const double *bh1, *left;   // diagonals [2, M]: BH1, and left_k of the slice being added
    int M, nbins, block, counter;
};

__global__ __launch_bounds__(TH_THREADS) void thermal_cslice_kernel(ThcSliceArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int M = a.M, LD = M | 1, tid = threadIdx.x, w = blockIdx.x;
    const size_t mat = ts_mat(M);
    cplx *V = (cplx *)smem, *T1 = V + mat, *T2 = T1 + mat;
    const long mm = (long)M * M;
    const cplx *Vw = a.vhs + (long)w * mm;
    // Horner: T_6 = I + V / 6, T_n = I + V T_{n + 1} / n, BV = T_1
    for (int e = tid; e < M * M; e += TH_THREADS) {
        const int r = e / M, c = e % M;
        const cplx x = Vw[e];
        V[r * LD + c] = x;
        T1[r * LD + c] = cmake(x.x / 6.0 + (r == c ? 1.0 : 0.0), x.y / 6.0);
    }
    __syncthreads();
    for (int n = 5; n >= 1; --n) {
        const double dn = (double)n;
        ts_gemm<cplx>(M, [&](int r, int k) { return V[r * LD + k]; }, [&](int k, int c) { return T1[k * LD + c]; },
                 [&](int r, int c, cplx x) { T2[r * LD + c] = cmake(x.x / dn + (r == c ? 1.0 : 0.0), x.y / dn); });
        __syncthreads();
        cplx *t = T1; T1 = T2; T2 = t;
    }
    const cplx *BV = T1;
    for (int s = 0; s < 2; ++s) {
        const double *d = a.bh1 + s * M, *lf = a.left + s * M;
        cplx *R = a.right + ((long)w * 2 + s) * mm;
        cplx *S = a.stack + (((long)w * a.nbins + a.block) * 2 + s) * mm;
        // B = diag(d) (BV diag(d)) as the reference forms it; right <- B right, right = I at the start of a bin
        if (a.counter == 0) {
            for (int e = tid; e < M * M; e += TH_THREADS) {
                const int r = e / M, c = e % M;
                T2[r * LD + c] = cscale(cscale(BV[r * LD + c], d[c]), d[r]);
            }
        } else {
            ts_gemm<cplx>(M, [&](int r, int k) { return cscale(cscale(BV[r * LD + k], d[k]), d[r]); },
                     [&](int k, int c) { return R[k * M + c]; }, [&](int r, int c, cplx x) { T2[r * LD + c] = x; });
        }
        __syncthreads();
        for (int e = tid; e < M * M; e += TH_THREADS) {
            const int r = e / M, c = e % M;
            const cplx x = T2[r * LD + c];
            R[e] = x;
            S[e] = cscale(x, lf[r]);
        }
        __syncthreads();
    }
}

// planewave.py:239-269 for one walker per work-group, whatever its weight: xbar = -sqrt(dt) vbias, a component with
// |xbar| > fb_bound scaled to unit modulus (counted in counters[0], as the ground-state field kernel counts its own),
// xs = xi - xbar, cmf = -sqrt(dt) xs . mf, cfb = xi . xbar - xbar . xbar / 2 (unconjugated).  Every thread sums its
// fields in order and the 256 partial sums are added in a fixed tree: the same bits on every run.
__global__ __launch_bounds__(TH_THREADS) void thermal_cfields_kernel(const cplx *vbias, const double *xi, const cplx *mf,
                                                                       cplx *xbar, cplx *xs, cplx *cmf, cplx *cfb, int K,
                                                                       double sqrt_dt, double fb_bound,
                                                                       unsigned long long *counters) {
    __shared__ double red[7][TH_THREADS];
    const int w = blockIdx.x, tid = threadIdx.x;
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};      // xs . mf (re, im), xi . xbar (re, im), xbar . xbar (re, im), clipped
    for (int n = tid; n < K; n += TH_THREADS) {
        const long e = (long)w * K + n;
        const cplx v = vbias[e], m = mf[n];
        cplx b = cmake(-sqrt_dt * v.x, -sqrt_dt * v.y);
        const double ab = hypot(b.x, b.y);
        if (ab > fb_bound) { b.x /= ab; b.y /= ab; acc[6] += 1.0; }
        const double x = xi[e];
        const cplx sft = cmake(x - b.x, -b.y);
        xbar[e] = b;
        xs[e] = sft;
        acc[0] += sft.x * m.x - sft.y * m.y;
        acc[1] += sft.x * m.y + sft.y * m.x;
        acc[2] += x * b.x; acc[3] += x * b.y;
        acc[4] += b.x * b.x - b.y * b.y;
        acc[5] += 2.0 * b.x * b.y;
    }
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

// planewave.py:493-517: oratio = M0_up M0_dn / (Mnew_up Mnew_dn), hyb = log(oratio) + cfb + cmf, magn = |exp(hyb)|;
// a zero denominator or a magn that is not finite: weight 0 and M0 kept; else weight *= magn max(0, cos arg exp(hyb - cfb)) and
// M0 <- Mnew (also when the cosine factor is 0).
__global__ void thermal_cweight_kernel(double *weight, cplx *M0, const cplx *Mnew, const cplx *cmf, const cplx *cfb, int nw) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    const cplx num = cmul(M0[2 * w], M0[2 * w + 1]), den = cmul(Mnew[2 * w], Mnew[2 * w + 1]);
    if (den.x == 0.0 && den.y == 0.0) { weight[w] = 0.0; return; }
    const cplx oratio = cdiv(num, den);
    const cplx lg = cmake(log(hypot(oratio.x, oratio.y)), atan2(oratio.y, oratio.x));
    const cplx hyb = cadd(cadd(lg, cfb[w]), cmf[w]);
    const double magn = exp(hyb.x);
    if (!(magn < INFINITY)) { weight[w] = 0.0; return; }      // infinite or NaN (a NaN M0 or Mnew): dies, keeps M0
    const double dtheta = hyb.y - cfb[w].y;
    const double cosine = fmax(0.0, cos(dtheta));
    weight[w] *= magn * cosine;
    M0[2 * w] = Mnew[2 * w];
    M0[2 * w + 1] = Mnew[2 * w + 1];
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

// One work-group per walker.  Per spin: B = BH1 (BV BH1) with the diagonal BV folded into the loader of the product's
// complex operand; right <- B right (right = B at in-bin counter 0); bin[block] = left_k right.
__global__ __launch_bounds__(TH_THREADS) void thermal_cslice_dense_kernel(ThdSliceArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int M = a.M, LD = M | 1, tid = threadIdx.x, w = blockIdx.x;
    const size_t mat = ts_mat(M);
    cplx *B = (cplx *)smem, *T2 = B + mat, *bv = T2 + mat;
    double *H = (double *)(bv + 64);
    const long mm = (long)M * M;
    if (tid < M) bv[tid] = a.bv[(long)w * M + tid];
    for (int s = 0; s < 2; ++s) {
        const double *Hs = a.bh1 + s * mm, *lf = a.left + s * mm;
        cplx *R = a.right + ((long)w * 2 + s) * mm;
        cplx *S = a.stack + (((long)w * a.nbins + a.block) * 2 + s) * mm;
        for (int e = tid; e < M * M; e += TH_THREADS) H[(e / M) * LD + e % M] = Hs[e];
        __syncthreads();
        thd_gemm_rc(M, [&](int r, int k) { return H[r * LD + k]; }, [&](int k, int c) { return cscale(bv[k], H[k * LD + c]); },
                    [&](int r, int c, cplx x) { B[r * LD + c] = x; });
        __syncthreads();
        const cplx *Rn = B;
        if (a.counter != 0) {
            ts_gemm<cplx>(M, [&](int r, int k) { return B[r * LD + k]; }, [&](int k, int c) { return R[k * M + c]; },
                          [&](int r, int c, cplx x) { T2[r * LD + c] = x; });
            __syncthreads();
            Rn = T2;
        }
        for (int e = tid; e < M * M; e += TH_THREADS) R[e] = Rn[(e / M) * LD + e % M];
        thd_gemm_rc(M, [&](int r, int k) { return lf[r * M + k]; }, [&](int k, int c) { return Rn[k * LD + c]; },
                    [&](int r, int c, cplx x) { S[r * M + c] = x; });
        __syncthreads();
    }
}

// continuous.py:97-115 with hubbard.py:241-250 for one walker per work-group, whatever its weight: vbias_i =
// i sqrt(U) (P_up,ii + P_dn,ii) from the diagonal of P [nw, 2, M, M], xbar = -sqrt(dt) (vbias - mf), a component with
// |xbar| > 1 scaled to unit modulus (each counted in counters[0]), xs, cmf, cfb as thermal_cfields_kernel makes them
// and in its order of summation, and the diagonal of BV: bv_i = sum_{n <= 6} v^n / n!, v = sqrt(dt) i sqrt(U) xs_i, by
// the reference's recurrence t <- v t / n.
__global__ __launch_bounds__(TH_THREADS) void thermal_cfields_dense_kernel(const cplx *P, const double *xi, const cplx *mf,
                                                                             cplx *xbar, cplx *xs, cplx *cmf, cplx *cfb,
                                                                             cplx *bv, int M, double sqrt_dt, double sqrt_u,
                                                                             unsigned long long *counters) {
    __shared__ double red[7][TH_THREADS];
    const int w = blockIdx.x, tid = threadIdx.x;
    const long mm = (long)M * M;
    const cplx *Pw = P + (long)w * 2 * mm;
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};      // xs . mf (re, im), xi . xbar (re, im), xbar . xbar (re, im), clipped
    for (int n = tid; n < M; n += TH_THREADS) {
        const long e = (long)w * M + n;
        const cplx pu = Pw[(long)n * M + n], pd = Pw[mm + (long)n * M + n], m = mf[n];
        const cplx v = cmake(-sqrt_u * (pu.y + pd.y), sqrt_u * (pu.x + pd.x));
        cplx b = cmake(-sqrt_dt * (v.x - m.x), -sqrt_dt * (v.y - m.y));
        const double ab = hypot(b.x, b.y);
        if (ab > 1.0) { b.x /= ab; b.y /= ab; acc[6] += 1.0; }
        const double x = xi[e];
        const cplx sft = cmake(x - b.x, -b.y);
        xbar[e] = b;
        xs[e] = sft;
        acc[0] += sft.x * m.x - sft.y * m.y;
        acc[1] += sft.x * m.y + sft.y * m.x;
        acc[2] += x * b.x; acc[3] += x * b.y;
        acc[4] += b.x * b.x - b.y * b.y;
        acc[5] += 2.0 * b.x * b.y;
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

// continuous.py:234-257: thermal_cweight_kernel with the constant of the mean-field shift: magn = |mfc exp(hyb)|
__global__ void thermal_cweight_mf_kernel(double *weight, cplx *M0, const cplx *Mnew, const cplx *cmf, const cplx *cfb,
                                          cplx mfc, int nw) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    const cplx num = cmul(M0[2 * w], M0[2 * w + 1]), den = cmul(Mnew[2 * w], Mnew[2 * w + 1]);
    if (den.x == 0.0 && den.y == 0.0) { weight[w] = 0.0; return; }
    const cplx oratio = cdiv(num, den);
    const cplx lg = cmake(log(hypot(oratio.x, oratio.y)), atan2(oratio.y, oratio.x));
    const cplx hyb = cadd(cadd(lg, cfb[w]), cmf[w]);
    const double ex = exp(hyb.x);
    const cplx eq = cmul(mfc, cmake(ex * cos(hyb.y), ex * sin(hyb.y)));
    const double magn = hypot(eq.x, eq.y);
    if (!(magn < INFINITY)) { weight[w] = 0.0; return; }      // infinite or NaN: dies, keeps M0
    const double dtheta = hyb.y - cfb[w].y;
    const double cosine = fmax(0.0, cos(dtheta));
    weight[w] *= magn * cosine;
    M0[2 * w] = Mnew[2 * w];
    M0[2 * w + 1] = Mnew[2 * w + 1];
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

// G and det of nblocks / 2 walkers by the engine the handle was configured with
static int thc_launch_greens(afq_handle *h, cplx *G, cplx *det, int first, int src_w, int nblocks) {
    if (h->thc_streamed)
        return ts_launch_greens_streamed<cplx>(h, h->thc_stack, G, det, h->thc_tscratch, first, src_w, nblocks);
    return ts_launch_greens<cplx>(h, h->thc_stack, G, det, first, src_w, nblocks);
}

int k_thermal_c_greens(afq_handle *h, int slice_ix) {
    return thc_launch_greens(h, h->thc_G, h->thc_det, ts_first_bin(h, slice_ix), -1, 2 * h->nw);
}

// walkers/handler.py:424-430: bins, G, weight.  The reference's reset leaves walker.M0 at the determinant the last path
// ended with, and the first slice of the next path divides by it: with_m0 (a fresh population) puts the trial's there.
int k_thermal_c_reset(afq_handle *h, bool with_m0) {
    const int M = h->M, nbins = h->th_nbins;
    const long per = 2L * M * M;
    // the trial's G and M0 once, from walker 0's fresh bins (every bin is BT^stack_size), then broadcast
    const double *BTpow = h->thc_dense ? h->thd_BTpow : h->thc_BTpow;
    const int dense = h->thc_dense ? 1 : 0;
    AFQ_LAUNCH(h, thermal_creset_kernel, dim3((unsigned)((per + 255) / 256), 1), dim3(256), 0, h->stream, h->thc_stack, h->thc_G,
               h->thc_right, h->thc_M0, h->weight, BTpow, h->thc_G0, h->thc_M00, nbins, M, 1, 0, dense);
    AFQ_POST(h);
    AFQ_TRY(thc_launch_greens(h, h->thc_G0, h->thc_M00, ts_first_bin(h, 0), 0, 2));
    AFQ_LAUNCH(h, thermal_creset_kernel, dim3((unsigned)((per + 255) / 256), h->nw), dim3(256), 0, h->stream, h->thc_stack,
               h->thc_G, h->thc_right, h->thc_M0, h->weight, BTpow, h->thc_G0, h->thc_M00, nbins, M, 0, with_m0 ? 1 : 0, dense);
    AFQ_POST(h);
    h->th_slice = 0; h->th_block = 0; h->th_counter = 0;
    return AFQ_OK;
}

int k_thermal_c_energy(afq_handle *h, double *E_out, double *nav_out) {
    AFQ_TRY(ts_launch_rdm<cplx>(h, h->thc_G, h->th_nav));
    if (h->thc_dense) {                                 // Hubbard: the full-G energy of P, as the real walkers' (k_thermal.hip)
        AFQ_TRY(k_energy_hubbard_full_g(h, h->G, h->nw, h->energy));
        return th_energy_out(h, E_out, nav_out);
    }
    cplx *two = nullptr, *E = nullptr;                  // (the per-q pair sums are scratch here)
    AFQ_TRY(k_ueg_sf_two(h, h->nw, &two, &E));
    AFQ_TRY(k_ueg_pair_sums(h, h->G, h->nw, h->energy, two));
    return th_energy_out(h, E_out, nav_out);
}

extern "C" {

int afq_thermal_configure_continuous(afq_handle *h, int ntime_slices, int stack_size, double dt, const double *BT,
                                     const double *BT_inv, const double *BH1, const double *mf_shift, double fb_bound,
                                     int options) {
    AFQ_API(h, "afq_thermal_configure_continuous");
    if (!h) return AFQ_EINVAL;
    h->th_on = false; h->th_cplx = false; h->thc_dense = false;
    if (!BT || !BT_inv || !BH1 || !mf_shift) AFQ_FAIL(h, AFQ_EINVAL, "afq_thermal_configure_continuous: null operand");
    if (options & AFQ_THERMAL_CHARGE) AFQ_FAIL(h, AFQ_EINVAL, "afq_thermal_configure_continuous: charge_decomposition belongs to the discrete fields");
    if (options & AFQ_THERMAL_FREE_PROJECTION) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: free_projection is not supported (constrained path only)");
    if (options & AFQ_THERMAL_LOW_RANK) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: low_rank is not supported");
    if (options & AFQ_THERMAL_AVERAGE_GF) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: average_gf is not supported");
    const bool streamed = (options & AFQ_THERMAL_STREAMED_GREENS) != 0;
    if (options & ~AFQ_THERMAL_STREAMED_GREENS) AFQ_FAIL(h, AFQ_EINVAL, "afq_thermal_configure_continuous: unknown option bits");
    if (!h->kind || !h->nw) AFQ_FAIL(h, AFQ_ESTATE, "afq_thermal_configure_continuous: set the system and allocate the walkers first");
    if (h->kind != AFQ_SYS_UEG) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers with continuous fields: UEG systems only (no Generic, no continuous Hubbard)");
    const int M = h->M;
    if (streamed) {
        // the smallest of what the slice kernel, the streamed Green's kernel and lane = column hold
        auto fits = [](int m) {
            return thc_slice_lds(m) <= THC_LDS_MAX && ts_greens_streamed_lds<cplx>(m) <= THC_LDS_MAX && m <= THC_LANES;
        };
        if (!fits(M)) {
            int mmax = M;
            while (mmax > 1 && !fits(mmax)) --mmax;
            const std::string head = "thermal walkers with continuous fields (streamed_greens): M = " + std::to_string(M) + " plane waves ";
            const std::string tail = " (M <= " + std::to_string(mmax) + ")";
            if (thc_slice_lds(M) > THC_LDS_MAX)
                AFQ_FAIL(h, AFQ_EUNSUPPORTED, head + "need " + std::to_string(thc_slice_lds(M)) + " bytes of LDS for the slice kernel "
                         "(thermal_cslice_kernel), a work-group has " + std::to_string(THC_LDS_MAX) + tail);
            if (ts_greens_streamed_lds<cplx>(M) > THC_LDS_MAX)
                AFQ_FAIL(h, AFQ_EUNSUPPORTED, head + "need " + std::to_string(ts_greens_streamed_lds<cplx>(M)) + " bytes of LDS for the "
                         "streamed Green's function (thermal_cgreens_streamed_kernel), a work-group has " + std::to_string(THC_LDS_MAX) + tail);
            AFQ_FAIL(h, AFQ_EUNSUPPORTED, head + "are more than the " + std::to_string(THC_LANES) + " lanes of a wave, one per column" + tail);
        }
    } else if (ts_greens_lds<cplx>(M) > THC_LDS_MAX) {
        int mmax = M;
        while (mmax > 1 && ts_greens_lds<cplx>(mmax) > THC_LDS_MAX) --mmax;
        AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers with continuous fields: M = " + std::to_string(M) + " plane waves need " +
                 std::to_string(ts_greens_lds<cplx>(M)) + " bytes of LDS for the complex Green's function, a work-group has " +
                 std::to_string(THC_LDS_MAX) + " (M <= " + std::to_string(mmax) + "); AFQ_THERMAL_STREAMED_GREENS (streamed_greens) "
                 "keeps T in device memory and reaches further");
    }
    if (k_comm_size(h) > 1) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: one rank only");
    if (h->nbp > 0 || h->it_nmax > 0) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: no back-propagation or ITCF window");
    if (h->rdm_on) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: no mixed one_rdm / two_rdm");
    if (ntime_slices < 1 || stack_size < 1 || ntime_slices % stack_size)
        AFQ_FAIL(h, AFQ_EINVAL, "afq_thermal_configure_continuous: stack_size must divide ntime_slices (both >= 1)");
    if (!(dt > 0.0) || !(fb_bound >= 0.0)) AFQ_FAIL(h, AFQ_EINVAL, "afq_thermal_configure_continuous: dt must be positive, fb_bound not negative");
    const size_t mm = (size_t)M * M, n = h->nw;
    for (int s = 0; s < 2; ++s)
        for (int i = 0; i < M; ++i)
            for (int j = 0; j < M; ++j)
                if (i != j && (BT[s * mm + (size_t)i * M + j] != 0.0 || BT_inv[s * mm + (size_t)i * M + j] != 0.0))
                    AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers with continuous fields: a diagonal trial density matrix only (OneBody on plane waves)");
    hipSetDevice(h->device);
    const int nbins = ntime_slices / stack_size;
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
    int rc;
    if ((rc = dev_upload(h, LT_WALKERS, &h->thc_BTpow, pw.data(), pw.size())) ||
        (rc = dev_upload(h, LT_WALKERS, &h->thc_left, left.data(), left.size())) ||
        (rc = dev_upload(h, LT_WALKERS, &h->thc_bh1, bh.data(), bh.size())) ||
        (rc = dev_upload(h, LT_WALKERS, &h->thc_mf, mf_shift, (size_t)h->K))) return rc;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->thc_G, 2 * mm * n)) || (rc = dev_alloc(h, LT_WALKERS, &h->thc_G0, 2 * mm)) ||
        (rc = dev_alloc(h, LT_WALKERS, &h->thc_stack, 2 * mm * n * nbins)) || (rc = dev_alloc(h, LT_WALKERS, &h->thc_right, 2 * mm * n)) ||
        (rc = dev_alloc(h, LT_WALKERS, &h->thc_M0, 2 * n)) || (rc = dev_alloc(h, LT_WALKERS, &h->thc_M00, (size_t)2)) ||
        (rc = dev_alloc(h, LT_WALKERS, &h->thc_det, 2 * n)) || (rc = dev_alloc(h, LT_WALKERS, &h->th_nav, n))) return rc;
    // T of the streamed Green's kernel, two buffers per (walker, spin); a handle configured without it holds none
    if ((rc = dev_alloc(h, LT_WALKERS, &h->thc_tscratch, streamed ? 4 * mm * n : (size_t)0))) return rc;
    h->thc_streamed = streamed;
    if ((rc = ensure_G(h))) return rc;                  // c128 [nw, 2, M, M]: the one-body density matrices
    h->thc_fb_bound = fb_bound;
    h->dt = dt; h->sqrt_dt = std::pow(dt, 0.5);        // (the handle's time step, as afq_set_propagator sets it)
    h->th_L = ntime_slices; h->th_ss = stack_size; h->th_nbins = nbins; h->th_nstblz = 1;
    h->th_on = true; h->th_cplx = true;
    return k_thermal_c_reset(h, true);
}

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
    h->th_on = false; h->th_cplx = false; h->thc_dense = false;
    const std::string me = "afq_thermal_configure_hubbard_continuous: ";
    if (!BT || !BT_inv || !BH1 || !mf_shift || !mf_const_fac) AFQ_FAIL(h, AFQ_EINVAL, me + "null operand");
    if (options & AFQ_THERMAL_CHARGE) AFQ_FAIL(h, AFQ_EINVAL, me + "charge_decomposition belongs to the discrete fields (the continuous form is the charge form alone)");
    if (options & AFQ_THERMAL_FREE_PROJECTION) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: free_projection is not supported (constrained path only)");
    if (options & AFQ_THERMAL_LOW_RANK) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: low_rank is not supported");
    if (options & AFQ_THERMAL_AVERAGE_GF) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: average_gf is not supported");
    const bool streamed = (options & AFQ_THERMAL_STREAMED_GREENS) != 0;
    if (options & ~AFQ_THERMAL_STREAMED_GREENS) AFQ_FAIL(h, AFQ_EINVAL, me + "unknown option bits");
    if (!h->kind || !h->nw) AFQ_FAIL(h, AFQ_ESTATE, me + "set the system and allocate the walkers first");
    if (h->kind != AFQ_SYS_HUBBARD) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers with continuous fields and a dense trial: Hubbard systems only (no Generic)");
    const int M = h->M;
    {
        // the smallest of what the slice kernel, the Green's kernel of the handle and lane = column hold
        auto greens_lds = [&](int m) { return streamed ? ts_greens_streamed_lds<cplx>(m) : ts_greens_lds<cplx>(m); };
        auto fits = [&](int m) { return thd_slice_lds(m) <= THC_LDS_MAX && greens_lds(m) <= THC_LDS_MAX && m <= THC_LANES; };
        if (!fits(M)) {
            int mmax = M;
            while (mmax > 1 && !fits(mmax)) --mmax;
            const std::string head = std::string("thermal walkers with continuous fields, Hubbard") + (streamed ? " (streamed_greens)" : "") +
                                     ": M = " + std::to_string(M) + " sites ";
            const std::string tail = " (M <= " + std::to_string(mmax) + ")";
            if (greens_lds(M) > THC_LDS_MAX)
                AFQ_FAIL(h, AFQ_EUNSUPPORTED, head + "need " + std::to_string(greens_lds(M)) + " bytes of LDS for the " +
                         (streamed ? "streamed Green's function (thermal_cgreens_streamed_kernel)"
                                   : "complex Green's function (thermal_cgreens_kernel)") +
                         ", a work-group has " + std::to_string(THC_LDS_MAX) + tail +
                         (streamed ? "" : "; AFQ_THERMAL_STREAMED_GREENS (streamed_greens) keeps T in device memory and reaches further"));
            if (thd_slice_lds(M) > THC_LDS_MAX)
                AFQ_FAIL(h, AFQ_EUNSUPPORTED, head + "need " + std::to_string(thd_slice_lds(M)) + " bytes of LDS for the slice kernel "
                         "(thermal_cslice_dense_kernel), a work-group has " + std::to_string(THC_LDS_MAX) + tail);
            AFQ_FAIL(h, AFQ_EUNSUPPORTED, head + "are more than the " + std::to_string(THC_LANES) + " lanes of a wave, one per column" + tail);
        }
    }
    if (k_comm_size(h) > 1) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: one rank only");
    if (h->nbp > 0 || h->it_nmax > 0) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: no back-propagation or ITCF window");
    if (h->rdm_on) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: no mixed one_rdm / two_rdm");
    if (ntime_slices < 1 || stack_size < 1 || ntime_slices % stack_size)
        AFQ_FAIL(h, AFQ_EINVAL, me + "stack_size must divide ntime_slices (both >= 1)");
    if (!(dt > 0.0)) AFQ_FAIL(h, AFQ_EINVAL, me + "dt must be positive");
    if (!(h->U >= 0.0)) AFQ_FAIL(h, AFQ_EINVAL, me + "U must not be negative (iu_fac = i sqrt(U))");
    hipSetDevice(h->device);
    const size_t mm = (size_t)M * M, n = h->nw;
    const int nbins = ntime_slices / stack_size;
    std::vector<double> pw(2 * mm), left((size_t)stack_size * 2 * mm);
    thd_left_table(M, stack_size, BT, BT_inv, pw.data(), left.data());
    int rc;
    if ((rc = dev_upload(h, LT_WALKERS, &h->thd_BTpow, pw.data(), pw.size())) ||
        (rc = dev_upload(h, LT_WALKERS, &h->thd_left, left.data(), left.size())) ||
        (rc = dev_upload(h, LT_WALKERS, &h->thd_bh1, BH1, 2 * mm)) ||
        (rc = dev_upload(h, LT_WALKERS, &h->thc_mf, mf_shift, (size_t)M))) return rc;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->thc_G, 2 * mm * n)) || (rc = dev_alloc(h, LT_WALKERS, &h->thc_G0, 2 * mm)) ||
        (rc = dev_alloc(h, LT_WALKERS, &h->thc_stack, 2 * mm * n * nbins)) || (rc = dev_alloc(h, LT_WALKERS, &h->thc_right, 2 * mm * n)) ||
        (rc = dev_alloc(h, LT_WALKERS, &h->thc_M0, 2 * n)) || (rc = dev_alloc(h, LT_WALKERS, &h->thc_M00, (size_t)2)) ||
        (rc = dev_alloc(h, LT_WALKERS, &h->thc_det, 2 * n)) || (rc = dev_alloc(h, LT_WALKERS, &h->th_nav, n))) return rc;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->thc_tscratch, streamed ? 4 * mm * n : (size_t)0))) return rc;
    h->thc_streamed = streamed;
    if ((rc = ensure_G(h))) return rc;                  // c128 [nw, 2, M, M]: the one-body density matrices
    h->thd_mf_const[0] = mf_const_fac[0]; h->thd_mf_const[1] = mf_const_fac[1];
    h->thd_sqrt_u = std::pow(h->U, 0.5);
    h->thc_fb_bound = 1.0;
    h->dt = dt; h->sqrt_dt = std::pow(dt, 0.5);
    h->th_L = ntime_slices; h->th_ss = stack_size; h->th_nbins = nbins; h->th_nstblz = 1;
    h->th_on = true; h->th_cplx = true; h->thc_dense = true;
    return k_thermal_c_reset(h, true);
}

int afq_thermal_propagate_continuous(afq_handle *h, const double *xi, double *xi_out) {
    AFQ_API(h, "afq_thermal_propagate_continuous");
    if (!h) return AFQ_EINVAL;
    AFQ_TRY(th_need(h, true));
    if (h->th_slice >= h->th_L) AFQ_FAIL(h, AFQ_ESTATE, "afq_thermal_propagate_continuous: the path is complete (afq_thermal_reset starts the next)");
    const int M = h->M;
    const size_t nf = (size_t)h->nw * h->K;
    // the fields of every walker, dead ones included (the thermal driver skips none): the host's, or the device stream
    if (xi) AFQ_HIP(h, hipMemcpyAsync(h->xi, xi, sizeof(double) * nf, hipMemcpyHostToDevice, h->stream));
    else AFQ_TRY(k_rng_normal_into(h, h->xi, (long)nf));
    if (h->thc_dense) {
        // P = I - G^T; the force bias, the clip at 1, xs, cmf, cfb and the diagonal of BV from P's diagonal
        AFQ_TRY(ts_launch_rdm<cplx>(h, h->thc_G, nullptr));
        AFQ_LAUNCH(h, thermal_cfields_dense_kernel, dim3(h->nw), dim3(TH_THREADS), 0, h->stream, h->G, h->xi, h->thc_mf,
                   h->xbar, h->xs, h->cmf, h->cfb, h->vhs, M, h->sqrt_dt, h->thd_sqrt_u, h->counters);
        AFQ_POST(h);
        ThdSliceArgs a;
        a.bv = h->vhs; a.right = h->thc_right; a.stack = h->thc_stack; a.bh1 = h->thd_bh1;
        a.left = h->thd_left + (size_t)h->th_counter * 2 * M * M;
        a.M = M; a.nbins = h->th_nbins; a.block = h->th_block; a.counter = h->th_counter;
        static size_t lds_set[AFQ_MAX_DEVICES] = {0};
        const size_t lds = thd_slice_lds(M);
        AFQ_HIP(h, afq_raise_lds((const void *)thermal_cslice_dense_kernel, lds, lds_set));
        AFQ_LAUNCH(h, thermal_cslice_dense_kernel, dim3(h->nw), dim3(TH_THREADS), lds, h->stream, a);
        AFQ_POST(h);
        h->th_slice += 1;
        h->th_block = h->th_slice / h->th_ss;
        h->th_counter = (h->th_counter + 1) % h->th_ss;
        AFQ_TRY(thc_launch_greens(h, h->thc_G, h->thc_det, 0, -1, 2 * h->nw));
        AFQ_LAUNCH(h, thermal_cweight_mf_kernel, dim3((h->nw + 127) / 128), dim3(128), 0, h->stream, h->weight, h->thc_M0,
                   h->thc_det, h->cmf, h->cfb, cmake(h->thd_mf_const[0], h->thd_mf_const[1]), h->nw);
        AFQ_POST(h);
        if (xi_out) return copy_out(h, xi_out, h->xi, sizeof(double) * nf);
        return AFQ_OK;
    }
    // P = I - G^T, vbias = P . [iA | iB], xbar = -sqrt(dt) vbias clipped at 1, xs, cmf, cfb (planewave.py:219-276)
    AFQ_TRY(ts_launch_rdm<cplx>(h, h->thc_G, nullptr));
    AFQ_TRY(k_vbias_ueg(h));
    AFQ_LAUNCH(h, thermal_cfields_kernel, dim3(h->nw), dim3(TH_THREADS), 0, h->stream, h->vbias, h->xi, h->thc_mf, h->xbar,
               h->xs, h->cmf, h->cfb, h->K, h->sqrt_dt, h->thc_fb_bound, h->counters);
    AFQ_POST(h);
    AFQ_TRY(k_vhs_ueg(h));                              // VHS = sqrt(dt) (iA xs[:nq] + iB xs[nq:])
    {
        ThcSliceArgs a;
        a.vhs = h->vhs; a.right = h->thc_right; a.stack = h->thc_stack; a.bh1 = h->thc_bh1;
        a.left = h->thc_left + (size_t)h->th_counter * 2 * M;
        a.M = M; a.nbins = h->th_nbins; a.block = h->th_block; a.counter = h->th_counter;
        static size_t lds_set[AFQ_MAX_DEVICES] = {0};
        const size_t lds = thc_slice_lds(M);
        AFQ_HIP(h, afq_raise_lds((const void *)thermal_cslice_kernel, lds, lds_set));
        AFQ_LAUNCH(h, thermal_cslice_kernel, dim3(h->nw), dim3(TH_THREADS), lds, h->stream, a);
        AFQ_POST(h);
    }
    // PropagatorStack.update_full_rank's counters (stack.py:322-324)
    h->th_slice += 1;
    h->th_block = h->th_slice / h->th_ss;
    h->th_counter = (h->th_counter + 1) % h->th_ss;
    // G = [I + S_{nbins - 1} .. S_0]^-1 on the walker's current bins, Mnew = det G, the weight
    AFQ_TRY(thc_launch_greens(h, h->thc_G, h->thc_det, 0, -1, 2 * h->nw));
    AFQ_LAUNCH(h, thermal_cweight_kernel, dim3((h->nw + 127) / 128), dim3(128), 0, h->stream, h->weight, h->thc_M0, h->thc_det,
               h->cmf, h->cfb, h->nw);
    AFQ_POST(h);
    if (xi_out) return copy_out(h, xi_out, h->xi, sizeof(double) * nf);
    return AFQ_OK;
}

}  // extern "C"
