// Finite-temperature AFQMC walkers with continuous Hubbard-Stratonovich fields for the uniform electron gas
// (thermal_propagation/planewave.py:219-276,445-517, walkers/stack.py:299-324, walkers/thermal.py:51-64,472-547 of the
// reference; phaseless path, force bias on, full-rank walkers, diagonal one-body trial density matrix).  Every matrix of
// the walker is complex: G_s c128 [2, M, M], the bins c128 [nbins, 2, M, M], the running product of the current bin
// `right` c128 [2, M, M] and M0_s = det G_s c128 [2].  The slice counter, the block and the in-bin counter are the
// handle's, as for the real walkers of k_thermal.hip.  A walker's working set stays in LDS: 4 complex matrices of pitch
// M | 1, which the 160 KiB of a compute unit hold up to M = 47 (the plane-wave shells: 7, 19, 27, 33; 57 does not fit).
//
//   thermal_cgreens_kernel  one work-group per (walker, spin): k_thermal.hip's stratified decomposition in complex
//                           arithmetic.  Q D T = B_first by column-pivoted QR with complex Householder reflectors
//                           H = I - tau v v^H (alpha = -x_0 / |x_0| ||x||, tau = (||x|| + |x_0|) / ||x|| real); per
//                           further bin C = (B Q) D, Q D t = C, T <- t T; D = D_b^-1 D_s split at |D| = 1
//                           (D_b = 1 / |D|, D_s = D / |D| where |D| > 1), (D_b Q^H + D_s T) G = D_b Q^H by one
//                           pivoted solve.  det G is the product of the pivots of an LU with partial pivoting of a
//                           copy of G in the matrix the solve has used up.  The products B Q and t T are complex
//                           products on v_mfma_f64_16x16x4f64, four real products each, edge tiles padded by zeros.
//   thermal_cslice_kernel   one work-group per walker: BV = sum_{n <= 6} VHS^n / n! by five Horner products in LDS,
//                           once for both spins; per spin B = diag(BH1) BV diag(BH1), right <- B right (right = I at
//                           in-bin counter 0), bin[block] = diag(left_k) right.
//   thermal_cweight_kernel  the phaseless weight update from the determinant ratio, per walker.
//   thermal_crdm_kernel     P_s = I - G_s^T for the force bias and the energy, nav = Re(tr P_up + tr P_down).
//   thermal_cfields_kernel  clip, shifted fields, cmf and cfb of every walker, dead ones included.
// The force bias and the HS potential are the plane-wave kernels of k_models.hip on P.
#include "afq_internal.h"
#include "afq_host.h"
#include "mfma_gemm.h"
#include <cmath>
#include <cstring>

#define THC_THREADS 256
#define THC_LDS_MAX (160 * 1024)

namespace {

// C = A B for complex M x M operands given as element loaders, by the 4 waves of the work-group: 16 x 16 tiles, k in
// steps of 4, four real MFMA products per step; rows, columns and k beyond M enter as zeros and are not stored.  The
// caller synchronises before and after.
template <class LA, class LB, class ST>
__device__ inline void thc_gemm(int M, LA la, LB lb, ST st) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const int nt = (M + 15) >> 4, lr = lane & 15, lk = lane >> 4;
    for (int tile = wave; tile < nt * nt; tile += nwave) {
        const int row0 = (tile / nt) << 4, col0 = (tile % nt) << 4;
        const int arow = row0 + lr, bcol = col0 + lr;
        d4_t re = (d4_t){0, 0, 0, 0}, im = (d4_t){0, 0, 0, 0};
        for (int k0 = 0; k0 < M; k0 += 4) {
            const int k = k0 + lk;
            const cplx a = (arow < M && k < M) ? la(arow, k) : cmake(0.0, 0.0);
            const cplx b = (bcol < M && k < M) ? lb(k, bcol) : cmake(0.0, 0.0);
            re = mfma16(a.x, b.x, re);
            re = mfma16(-a.y, b.y, re);
            im = mfma16(a.x, b.y, im);
            im = mfma16(a.y, b.x, im);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + lk + 4 * r;
            if (row < M && bcol < M) st(row, bcol, cmake(re[r], im[r]));
        }
    }
}

// (value, index) of the largest val over the 64 lanes of a wave; ties go to the lower index; every lane gets the result
__device__ inline void thc_wave_argmax(double &val, int &idx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(val, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ov > val || (ov == val && oi < idx)) { val = ov; idx = oi; }
    }
}

__device__ inline cplx thc_sum4(const cplx *p) {
    return cadd(cadd(p[0], p[64]), cadd(p[128], p[192]));
}

// Column-pivoted Householder QR of the complex W [M, M] (LDS, row-major, leading dimension LD), in place: W P = Q R.
// On return the upper triangle of W holds R (zeros below), perm[j] the original column now at position j, Qt = Q^H.
// The pivot of step j is the remaining column of the largest norm over the rows j.., recomputed every step.
// part: 8 * 64 complex, v: 64 complex.  Every wave runs the pivot search on its own: no shared scalars.
__device__ void thc_qrcp(cplx *W, cplx *Qt, int M, int LD, int *perm, cplx *v, cplx *part) {
    const int tid = threadIdx.x, c = tid & 63, q = tid >> 6;
    for (int e = tid; e < M * M; e += THC_THREADS) { const int r = e / M, cc = e % M; Qt[r * LD + cc] = cmake(r == cc ? 1.0 : 0.0, 0.0); }
    if (tid < M) perm[tid] = tid;
    __syncthreads();
    for (int j = 0; j < M; ++j) {
        if (c >= j && c < M) {
            double s = 0.0;
            for (int i = j + q; i < M; i += 4) { const cplx x = W[i * LD + c]; s = fma(x.x, x.x, s); s = fma(x.y, x.y, s); }
            part[q * 64 + c].x = s;
        }
        __syncthreads();
        double nrm2 = (c >= j && c < M) ? (part[c].x + part[64 + c].x) + (part[128 + c].x + part[192 + c].x) : -1.0;
        int piv = c;
        thc_wave_argmax(nrm2, piv);
        if (piv != j) {
            if (tid < M) { const cplx t = W[tid * LD + j]; W[tid * LD + j] = W[tid * LD + piv]; W[tid * LD + piv] = t; }
            if (tid == THC_THREADS - 1) { const int t = perm[j]; perm[j] = perm[piv]; perm[piv] = t; }
        }
        __syncthreads();
        const cplx x0 = W[j * LD + j];
        const double nrm = sqrt(nrm2), ax0 = hypot(x0.x, x0.y);
        const cplx ph = ax0 > 0.0 ? cmake(x0.x / ax0, x0.y / ax0) : cmake(1.0, 0.0);
        const cplx alpha = cmake(-ph.x * nrm, -ph.y * nrm);          // H x = alpha e_0, |x_0 - alpha| = |x_0| + ||x||
        const double tau = nrm > 0.0 ? (nrm + ax0) / nrm : 0.0;
        const cplx den = cmake(ph.x * (ax0 + nrm), ph.y * (ax0 + nrm));   // x_0 - alpha
        if (tid < M - j)
            v[j + tid] = (tid == 0 || !(nrm > 0.0)) ? cmake(tid == 0 ? 1.0 : 0.0, 0.0) : cdiv(W[(j + tid) * LD + j], den);
        __syncthreads();
        // v^H W[:, c] for the trailing columns and v^H Qt[:, c] for every column, four row classes per column
        if (c < M) {
            cplx sw = cmake(0.0, 0.0), sq = cmake(0.0, 0.0);
            for (int i = j + q; i < M; i += 4) {
                const cplx vc = cconj(v[i]);
                if (c > j) cfma(sw, vc, W[i * LD + c]);
                cfma(sq, vc, Qt[i * LD + c]);
            }
            part[q * 64 + c] = sw; part[256 + q * 64 + c] = sq;
        }
        __syncthreads();
        if (c < M) {
            const cplx sw = cscale(thc_sum4(part + c), -tau), sq = cscale(thc_sum4(part + 256 + c), -tau);
            for (int i = j + q; i < M; i += 4) {
                const cplx vi = v[i];
                if (c > j) cfma(W[i * LD + c], sw, vi);
                cfma(Qt[i * LD + c], sq, vi);
            }
            if (c == j && nrm > 0.0) for (int i = j + q; i < M; i += 4) W[i * LD + j] = i == j ? alpha : cmake(0.0, 0.0);
        }
        __syncthreads();
    }
}

// X G = R for complex X, R [M, M] in LDS by Gauss-Jordan elimination with partial (row) pivoting; G overwrites R, X is
// destroyed.  colv, rowx, rowr: 64 complex each.
__device__ void thc_solve(cplx *X, cplx *R, int M, int LD, cplx *colv, cplx *rowx, cplx *rowr) {
    const int tid = threadIdx.x, c = tid & 63;
    for (int k = 0; k < M; ++k) {
        double a = -1.0;
        if (c >= k && c < M) { const cplx x = X[c * LD + k]; a = hypot(x.x, x.y); }
        int p = c;
        thc_wave_argmax(a, p);
        __syncthreads();                                  // (every wave has read column k before rows move)
        if (p != k) {
            if (tid < M) { const cplx t = X[k * LD + tid]; X[k * LD + tid] = X[p * LD + tid]; X[p * LD + tid] = t; }
            else if (tid >= 64 && tid < 64 + M) { const cplx t = R[k * LD + c]; R[k * LD + c] = R[p * LD + c]; R[p * LD + c] = t; }
        }
        __syncthreads();
        const cplx piv = X[k * LD + k];
        __syncthreads();
        if (tid < M) { colv[tid] = X[tid * LD + k]; rowx[tid] = cdiv(X[k * LD + tid], piv); }
        else if (tid >= 64 && tid < 64 + M) rowr[c] = cdiv(R[k * LD + c], piv);
        __syncthreads();
        for (int e = tid; e < M * M; e += THC_THREADS) {
            const int i = e / M, cc = e % M;
            if (i == k) { X[i * LD + cc] = rowx[cc]; R[i * LD + cc] = rowr[cc]; }
            else {
                const cplx f = cmake(-colv[i].x, -colv[i].y);
                cfma(X[i * LD + cc], f, rowx[cc]);
                cfma(R[i * LD + cc], f, rowr[cc]);
            }
        }
        __syncthreads();
    }
}

// det X of the complex X [M, M] in LDS: the product of the pivots of an LU with partial (row) pivoting, the sign of every
// row exchange included; X is destroyed.  Every thread returns the same value.  colv: 64 complex.
__device__ cplx thc_det(cplx *X, int M, int LD, cplx *colv) {
    const int tid = threadIdx.x, c = tid & 63;
    cplx det = cmake(1.0, 0.0);
    for (int k = 0; k < M; ++k) {
        double a = -1.0;
        if (c >= k && c < M) { const cplx x = X[c * LD + k]; a = hypot(x.x, x.y); }
        int p = c;
        thc_wave_argmax(a, p);
        __syncthreads();
        if (p != k) {
            if (tid < M) { const cplx t = X[k * LD + tid]; X[k * LD + tid] = X[p * LD + tid]; X[p * LD + tid] = t; }
            det = cmake(-det.x, -det.y);
        }
        __syncthreads();
        const cplx piv = X[k * LD + k];                   // (the same value in every thread: uniform branches below)
        det = cmul(det, piv);
        if (piv.x == 0.0 && piv.y == 0.0) return cmake(0.0, 0.0);
        if (tid > k && tid < M) colv[tid] = cdiv(X[tid * LD + k], piv);
        __syncthreads();
        const int n = M - k - 1;
        for (int e = tid; e < n * n; e += THC_THREADS) {
            const int i = k + 1 + e / n, cc = k + 1 + e % n;
            cfma(X[i * LD + cc], cmake(-colv[i].x, -colv[i].y), X[k * LD + cc]);
        }
        __syncthreads();
    }
    return det;
}

__host__ __device__ inline size_t thc_mat(int M) { return (size_t)M * (M | 1); }
// LDS of the Green's kernel: 4 matrices, D[64], v[64], part[512], aux[192] complex, perm[64]
inline size_t thc_greens_lds(int M) { return sizeof(cplx) * (4 * thc_mat(M) + 64 + 64 + 512 + 192) + sizeof(int) * 64; }
inline size_t thc_slice_lds(int M) { return sizeof(cplx) * 3 * thc_mat(M); }

// G[w, s] and det G[w, s] from the bins of walker w in the order first, first + 1, .. (mod nbins).
// stack [nw, nbins, 2, M, M]; src_w < 0: block b works on walker b / 2, otherwise every block works on walker src_w and
// writes walker 0's place (grid of 2 blocks).  det may be null.
__global__ __launch_bounds__(THC_THREADS) void thermal_cgreens_kernel(const cplx *stack, cplx *G, cplx *det, int M, int nbins,
                                                                       int first, int src_w) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int LD = M | 1, tid = threadIdx.x;
    const size_t mat = thc_mat(M);
    cplx *W = (cplx *)smem, *Qt = W + mat, *T = Qt + mat, *X = T + mat;
    cplx *D = X + mat, *v = D + 64, *part = v + 64, *aux = part + 512;
    int *perm = (int *)(aux + 192);
    const int w = src_w < 0 ? blockIdx.x >> 1 : src_w, s = blockIdx.x & 1;
    const long mm = (long)M * M;
    const cplx *Bw = stack + ((long)w * nbins * 2 + s) * mm;         // bin b at Bw + b * 2 * mm

    {
        const cplx *B = Bw + (long)first * 2 * mm;
        for (int e = tid; e < M * M; e += THC_THREADS) W[(e / M) * LD + e % M] = B[e];
    }
    __syncthreads();
    thc_qrcp(W, Qt, M, LD, perm, v, part);
    // T = D^-1 R P^T
    for (int e = tid; e < M * M; e += THC_THREADS) {
        const int i = e / M, j = e % M;
        T[i * LD + perm[j]] = j >= i ? cdiv(W[i * LD + j], W[i * LD + i]) : cmake(0.0, 0.0);
    }
    if (tid < M) D[tid] = W[tid * LD + tid];
    __syncthreads();
    for (int n = 1; n < nbins; ++n) {
        const cplx *B = Bw + (long)((first + n) % nbins) * 2 * mm;
        // W = (B Q) D, Q[k][c] = conj(Qt[c][k])
        thc_gemm(M, [&](int r, int k) { return B[r * M + k]; }, [&](int k, int c) { return cconj(Qt[c * LD + k]); },
                 [&](int r, int c, cplx x) { W[r * LD + c] = cmul(x, D[c]); });
        __syncthreads();
        thc_qrcp(W, Qt, M, LD, perm, v, part);
        for (int e = tid; e < M * M; e += THC_THREADS) {
            const int i = e / M, j = e % M;
            X[i * LD + perm[j]] = j >= i ? cdiv(W[i * LD + j], W[i * LD + i]) : cmake(0.0, 0.0);
        }
        if (tid < M) D[tid] = W[tid * LD + tid];
        __syncthreads();
        // T <- t T (into W, whose R is used up; then the two change names)
        thc_gemm(M, [&](int r, int k) { return X[r * LD + k]; }, [&](int k, int c) { return T[k * LD + c]; },
                 [&](int r, int c, cplx x) { W[r * LD + c] = x; });
        __syncthreads();
        cplx *t = T; T = W; W = t;
    }
    // (D_b Q^H + D_s T) G = D_b Q^H, D_b = 1 / |D| and D_s = D / |D| where |D| > 1, else D_b = 1 and D_s = D
    for (int e = tid; e < M * M; e += THC_THREADS) {
        const int i = e / M, j = e % M;
        const cplx d = D[i];
        const double ad = hypot(d.x, d.y);
        const double db = ad > 1.0 ? 1.0 / ad : 1.0;
        const cplx ds = ad > 1.0 ? cmake(d.x / ad, d.y / ad) : d;
        const cplx r = cscale(Qt[i * LD + j], db);
        cplx x = r;
        cfma(x, ds, T[i * LD + j]);
        X[i * LD + j] = x;
        W[i * LD + j] = r;
    }
    __syncthreads();
    thc_solve(X, W, M, LD, aux, aux + 64, aux + 128);
    const long slot = (long)(src_w < 0 ? w : 0) * 2 + s;
    cplx *Gd = G + slot * mm;
    for (int e = tid; e < M * M; e += THC_THREADS) {
        const cplx g = W[(e / M) * LD + e % M];
        Gd[e] = g;
        X[(e / M) * LD + e % M] = g;
    }
    if (!det) return;
    __syncthreads();
    const cplx dg = thc_det(X, M, LD, aux);
    if (tid == 0) det[slot] = dg;
}

struct ThcSliceArgs {
    const cplx *vhs;            // [nw, M, M]
    cplx *right, *stack;        // [nw, 2, M, M], [nw, nbins, 2, M, M]
    const double *bh1, *left;   // diagonals [2, M]: BH1, and left_k of the slice being added
    int M, nbins, block, counter;
};

__global__ __launch_bounds__(THC_THREADS) void thermal_cslice_kernel(ThcSliceArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int M = a.M, LD = M | 1, tid = threadIdx.x, w = blockIdx.x;
    const size_t mat = thc_mat(M);
    cplx *V = (cplx *)smem, *T1 = V + mat, *T2 = T1 + mat;
    const long mm = (long)M * M;
    const cplx *Vw = a.vhs + (long)w * mm;
    // Horner: T_6 = I + V / 6, T_n = I + V T_{n + 1} / n, BV = T_1
    for (int e = tid; e < M * M; e += THC_THREADS) {
        const int r = e / M, c = e % M;
        const cplx x = Vw[e];
        V[r * LD + c] = x;
        T1[r * LD + c] = cmake(x.x / 6.0 + (r == c ? 1.0 : 0.0), x.y / 6.0);
    }
    __syncthreads();
    for (int n = 5; n >= 1; --n) {
        const double dn = (double)n;
        thc_gemm(M, [&](int r, int k) { return V[r * LD + k]; }, [&](int k, int c) { return T1[k * LD + c]; },
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
            for (int e = tid; e < M * M; e += THC_THREADS) {
                const int r = e / M, c = e % M;
                T2[r * LD + c] = cscale(cscale(BV[r * LD + c], d[c]), d[r]);
            }
        } else {
            thc_gemm(M, [&](int r, int k) { return cscale(cscale(BV[r * LD + k], d[k]), d[r]); },
                     [&](int k, int c) { return R[k * M + c]; }, [&](int r, int c, cplx x) { T2[r * LD + c] = x; });
        }
        __syncthreads();
        for (int e = tid; e < M * M; e += THC_THREADS) {
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
__global__ __launch_bounds__(THC_THREADS) void thermal_cfields_kernel(const cplx *vbias, const double *xi, const cplx *mf,
                                                                       cplx *xbar, cplx *xs, cplx *cmf, cplx *cfb, int K,
                                                                       double sqrt_dt, double fb_bound,
                                                                       unsigned long long *counters) {
    __shared__ double red[7][THC_THREADS];
    const int w = blockIdx.x, tid = threadIdx.x;
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};      // xs . mf (re, im), xi . xbar (re, im), xbar . xbar (re, im), clipped
    for (int n = tid; n < K; n += THC_THREADS) {
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
    for (int o = THC_THREADS / 2; o > 0; o >>= 1) {
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

// P_s = I - G_s^T [nw, 2, M, M] for the force bias and the energy, nav = Re(tr P_up + tr P_down) (nav may be null)
__global__ __launch_bounds__(THC_THREADS) void thermal_crdm_kernel(const cplx *G, cplx *P, double *nav, int M) {
    __shared__ double red[THC_THREADS];
    const int w = blockIdx.x, tid = threadIdx.x;
    const long mm = (long)M * M;
    const cplx *Gw = G + (long)w * 2 * mm;
    cplx *Pw = P + (long)w * 2 * mm;
    for (int e = tid; e < 2 * M * M; e += THC_THREADS) {
        const int s = e / (M * M), r = (e / M) % M, c = e % M;
        const cplx g = Gw[s * mm + (long)c * M + r];
        Pw[e] = cmake((r == c ? 1.0 : 0.0) - g.x, -g.y);
    }
    if (!nav) return;
    double t = 0.0;
    for (int e = tid; e < 2 * M; e += THC_THREADS) t += 1.0 - Gw[(e / M) * mm + (long)(e % M) * M + e % M].x;
    red[tid] = t;
    __syncthreads();
    for (int o = THC_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) nav[w] = red[0];
}

// walker blockIdx.y: bins <- diag(BTpow) [2, M]; unless bins_only also G <- G0, right <- I, weight <- 1, and with_m0
// M0 <- M00
__global__ void thermal_creset_kernel(cplx *stack, cplx *G, cplx *right, cplx *M0, double *weight, const double *BTpow,
                                      const cplx *G0, const cplx *M00, int nbins, int M, int bins_only, int with_m0) {
    const long per = 2L * M * M;
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const int w = blockIdx.y;
    if (i < per) {
        const int s = (int)(i / ((long)M * M)), r = (int)((i / M) % M), c = (int)(i % M);
        const cplx b = cmake(r == c ? BTpow[s * M + r] : 0.0, 0.0);
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

int thc_launch_greens(afq_handle *h, const cplx *stack, cplx *G, cplx *det, int first, int src_w, int nblocks) {
    static size_t lds_set[AFQ_MAX_DEVICES] = {0};
    const size_t lds = thc_greens_lds(h->M);
    AFQ_HIP(h, afq_raise_lds((const void *)thermal_cgreens_kernel, lds, lds_set));
    AFQ_LAUNCH(h, thermal_cgreens_kernel, dim3(nblocks), dim3(THC_THREADS), lds, h->stream, stack, G, det, h->M, h->th_nbins,
               first, src_w);
    AFQ_POST(h);
    return AFQ_OK;
}

int thc_first_bin(const afq_handle *h, int slice_ix) {
    int bin_ix = slice_ix / h->th_ss;
    if (bin_ix == h->th_nbins) bin_ix = -1;
    return (bin_ix + 1) % h->th_nbins;
}

int thc_need(afq_handle *h) {
    if (!h->th_on || !h->th_cplx || !h->nw) AFQ_FAIL(h, AFQ_ESTATE, "thermal walkers: afq_thermal_configure_continuous first");
    if (h->prop_pending) AFQ_FAIL(h, AFQ_ESTATE, "a step is half done: afq_propagate_finish first");
    hipSetDevice(h->device);
    return AFQ_OK;
}

}  // namespace

int k_thermal_c_greens(afq_handle *h, int slice_ix) {
    return thc_launch_greens(h, h->thc_stack, h->thc_G, h->thc_det, thc_first_bin(h, slice_ix), -1, 2 * h->nw);
}

// walkers/handler.py:424-430: bins, G, weight.  The reference's reset leaves walker.M0 at the determinant the last path
// ended with, and the first slice of the next path divides by it: with_m0 (a fresh population) puts the trial's there.
int k_thermal_c_reset(afq_handle *h, bool with_m0) {
    const int M = h->M, nbins = h->th_nbins;
    const long per = 2L * M * M;
    // the trial's G and M0 once, from walker 0's fresh bins (every bin is BT^stack_size), then broadcast
    AFQ_LAUNCH(h, thermal_creset_kernel, dim3((unsigned)((per + 255) / 256), 1), dim3(256), 0, h->stream, h->thc_stack, h->thc_G,
               h->thc_right, h->thc_M0, h->weight, h->thc_BTpow, h->thc_G0, h->thc_M00, nbins, M, 1, 0);
    AFQ_POST(h);
    AFQ_TRY(thc_launch_greens(h, h->thc_stack, h->thc_G0, h->thc_M00, thc_first_bin(h, 0), 0, 2));
    AFQ_LAUNCH(h, thermal_creset_kernel, dim3((unsigned)((per + 255) / 256), h->nw), dim3(256), 0, h->stream, h->thc_stack,
               h->thc_G, h->thc_right, h->thc_M0, h->weight, h->thc_BTpow, h->thc_G0, h->thc_M00, nbins, M, 0, with_m0 ? 1 : 0);
    AFQ_POST(h);
    h->th_slice = 0; h->th_block = 0; h->th_counter = 0;
    return AFQ_OK;
}

int k_thermal_c_energy(afq_handle *h, double *E_out, double *nav_out) {
    AFQ_LAUNCH(h, thermal_crdm_kernel, dim3(h->nw), dim3(THC_THREADS), 0, h->stream, h->thc_G, h->G, h->th_nav, h->M);
    AFQ_POST(h);
    cplx *two = nullptr, *E = nullptr;                  // (the per-q pair sums are scratch here)
    AFQ_TRY(k_ueg_sf_two(h, h->nw, &two, &E));
    AFQ_TRY(k_ueg_pair_sums(h, h->G, h->nw, h->energy, two));
    if (E_out) {
        std::vector<double> e(6 * (size_t)h->nw);
        AFQ_TRY(copy_out(h, e.data(), h->energy, sizeof(cplx) * 3 * (size_t)h->nw));
        for (size_t i = 0; i < 3 * (size_t)h->nw; ++i) E_out[i] = e[2 * i];
    }
    return copy_out(h, nav_out, h->th_nav, sizeof(double) * (size_t)h->nw);
}

extern "C" {

int afq_thermal_configure_continuous(afq_handle *h, int ntime_slices, int stack_size, double dt, const double *BT,
                                     const double *BT_inv, const double *BH1, const double *mf_shift, double fb_bound,
                                     int options) {
    AFQ_API(h, "afq_thermal_configure_continuous");
    if (!h) return AFQ_EINVAL;
    h->th_on = false; h->th_cplx = false;
    if (!BT || !BT_inv || !BH1 || !mf_shift) AFQ_FAIL(h, AFQ_EINVAL, "afq_thermal_configure_continuous: null operand");
    if (options & AFQ_THERMAL_CHARGE) AFQ_FAIL(h, AFQ_EINVAL, "afq_thermal_configure_continuous: charge_decomposition belongs to the discrete fields");
    if (options & AFQ_THERMAL_FREE_PROJECTION) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: free_projection is not supported (constrained path only)");
    if (options & AFQ_THERMAL_LOW_RANK) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: low_rank is not supported");
    if (options & AFQ_THERMAL_AVERAGE_GF) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: average_gf is not supported");
    if (options) AFQ_FAIL(h, AFQ_EINVAL, "afq_thermal_configure_continuous: unknown option bits");
    if (!h->kind || !h->nw) AFQ_FAIL(h, AFQ_ESTATE, "afq_thermal_configure_continuous: set the system and allocate the walkers first");
    if (h->kind != AFQ_SYS_UEG) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers with continuous fields: UEG systems only (no Generic, no continuous Hubbard)");
    const int M = h->M;
    if (thc_greens_lds(M) > THC_LDS_MAX) {
        int mmax = M;
        while (mmax > 1 && thc_greens_lds(mmax) > THC_LDS_MAX) --mmax;
        AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers with continuous fields: M = " + std::to_string(M) + " plane waves need " +
                 std::to_string(thc_greens_lds(M)) + " bytes of LDS for the complex Green's function, a work-group has " +
                 std::to_string(THC_LDS_MAX) + " (M <= " + std::to_string(mmax) + ")");
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
    if ((rc = ensure_G(h))) return rc;                  // c128 [nw, 2, M, M]: the one-body density matrices
    h->thc_fb_bound = fb_bound;
    h->dt = dt; h->sqrt_dt = std::pow(dt, 0.5);        // (the handle's time step, as afq_set_propagator sets it)
    h->th_L = ntime_slices; h->th_ss = stack_size; h->th_nbins = nbins; h->th_nstblz = 1;
    h->th_on = true; h->th_cplx = true;
    return k_thermal_c_reset(h, true);
}

int afq_thermal_propagate_continuous(afq_handle *h, const double *xi, double *xi_out) {
    AFQ_API(h, "afq_thermal_propagate_continuous");
    if (!h) return AFQ_EINVAL;
    AFQ_TRY(thc_need(h));
    if (h->th_slice >= h->th_L) AFQ_FAIL(h, AFQ_ESTATE, "afq_thermal_propagate_continuous: the path is complete (afq_thermal_reset starts the next)");
    const int M = h->M;
    const size_t nf = (size_t)h->nw * h->K;
    // the fields of every walker, dead ones included (the thermal driver skips none): the host's, or the device stream
    if (xi) AFQ_HIP(h, hipMemcpyAsync(h->xi, xi, sizeof(double) * nf, hipMemcpyHostToDevice, h->stream));
    else AFQ_TRY(k_rng_normal_into(h, h->xi, (long)nf));
    // P = I - G^T, vbias = P . [iA | iB], xbar = -sqrt(dt) vbias clipped at 1, xs, cmf, cfb (planewave.py:219-276)
    AFQ_LAUNCH(h, thermal_crdm_kernel, dim3(h->nw), dim3(THC_THREADS), 0, h->stream, h->thc_G, h->G, (double *)nullptr, M);
    AFQ_POST(h);
    AFQ_TRY(k_vbias_ueg(h));
    AFQ_LAUNCH(h, thermal_cfields_kernel, dim3(h->nw), dim3(THC_THREADS), 0, h->stream, h->vbias, h->xi, h->thc_mf, h->xbar,
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
        AFQ_LAUNCH(h, thermal_cslice_kernel, dim3(h->nw), dim3(THC_THREADS), lds, h->stream, a);
        AFQ_POST(h);
    }
    // PropagatorStack.update_full_rank's counters (stack.py:322-324)
    h->th_slice += 1;
    h->th_block = h->th_slice / h->th_ss;
    h->th_counter = (h->th_counter + 1) % h->th_ss;
    // G = [I + S_{nbins - 1} .. S_0]^-1 on the walker's current bins, Mnew = det G, the weight
    AFQ_TRY(thc_launch_greens(h, h->thc_stack, h->thc_G, h->thc_det, 0, -1, 2 * h->nw));
    AFQ_LAUNCH(h, thermal_cweight_kernel, dim3((h->nw + 127) / 128), dim3(128), 0, h->stream, h->weight, h->thc_M0, h->thc_det,
               h->cmf, h->cfb, h->nw);
    AFQ_POST(h);
    if (xi_out) return copy_out(h, xi_out, h->xi, sizeof(double) * nf);
    return AFQ_OK;
}

}  // extern "C"
