// Pair sums of the UEG energy on GENERAL Green's functions, kept per momentum transfer (estimators/ueg.py:27-88):
//   Gkpq[s,q]  = sum_a G_s[kpq_i[q][a], kpq[q][a]]        Gpmq[s,q] = sum_b G_s[pmq_i[q][b], pmq[q][b]]
//   Gprod[s,q] = sum_{a,b} G_s[pmq_i[q][b], kpq[q][a]] G_s[kpq_i[q][a], pmq[q][b]]
//   two_rdm[s,s,q] = Gkpq[s,q] Gpmq[s,q] - Gprod[s,q]     two_rdm[s,t,q] = Gkpq[s,q] Gpmq[t,q]  (s != t)
//   ke = sum_s sum_i H1[s,i,i] G_s[i,i]                   pe = 1 / (2 vol) sum_q vqvec[q] sum_{s,t} two_rdm[s,t,q]
// energy_ueg_kernel / energy_ueg_q_kernel (k_models.hip) compute the same sums for the walkers' mixed Green's functions,
// whose only non-zero rows are the trial's, and fold them into one energy.  Here G is any matrix (the back-propagated
// G_bp has dense rows) and the per-q values are the result: the structure factor's two_rdm[2, 2, nq].
//
// ueg_pair_kernel: one work-group per (Green's function, spin).  The spin block goes to LDS whole when it fits
// (16 M P bytes, P = M | 1: an odd pitch spreads a column gather over the 16 slots a ds_read_b128 group of 16 lanes
// shares), else only the rows the lists name when those fit, else the gathers read global memory.  Momentum transfers
// are dealt by cost nk * np, not by q: `order` lists them by decreasing cost, the first `nlong` (cost > 64) go to the
// waves in turn, lanes over the (a, b) pairs, the rest -- the short and the empty lists -- one per thread.
// ueg_pair_finish_kernel: cross-spin products, ke, pe per Green's function.  ueg_sf_wsum_kernel: sum over Green's
// functions in index order, one thread per element: no atomics, the same bits on every run.
// hubbard_energy_full_g_kernel: estimators/hubbard.py:93-114 on full Green's functions.
#include "afq_internal.h"

namespace {

constexpr int SF_THREADS = 1024;
constexpr size_t SF_LDS_MAX = 156 * 1024;      // of the 160 KiB of a CU; the static arrays and the runtime keep the rest

// MODE 0: spin block in LDS (raw rows), 1: the lists' rows in LDS (compact rows), 2: global gathers (raw rows, P = M)
template <int MODE>
__global__ __launch_bounds__(SF_THREADS) void ueg_pair_kernel(const cplx *G, cplx *part, int M, int nq, int P,
                                                              const int *koff, const int *kp, const int *poff,
                                                              const int *pm, const int *rows, int nrows,
                                                              const int *order, int nlong) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int g = blockIdx.x >> 1, s = blockIdx.x & 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwave = blockDim.x >> 6;
    const cplx *Gg = G + ((long)g * 2 + s) * M * M;
    cplx *st = (cplx *)smem;
    if (MODE == 0) {
        for (int e = tid; e < M * M; e += (int)blockDim.x) {
            const int r = e / M, c = e - r * M;
            st[r * P + c] = Gg[e];
        }
    } else if (MODE == 1) {
        for (int e = tid; e < nrows * M; e += (int)blockDim.x) {
            const int r = e / M, c = e - r * M;
            st[r * P + c] = Gg[(long)rows[r] * M + c];
        }
    }
    if (MODE != 2) __syncthreads();
    auto at = [&](int r, int c) -> cplx {
        if constexpr (MODE == 2) return Gg[(long)r * M + c];
        else return st[r * P + c];
    };
    cplx *out = part + ((long)g * 2 + s) * nq * 3;
    // long lists: a wave per momentum transfer, lanes over the nk * np pairs
    for (int j = wave; j < nlong; j += nwave) {
        const int q = order[j];
        const int k0 = koff[q], nk = koff[q + 1] - k0, p0 = poff[q], np = poff[q + 1] - p0;    // nk * np > 64: np >= 1
        double ar = 0, ai = 0, br = 0, bi = 0, cr = 0, ci = 0;
        for (int z = lane; z < nk; z += 64) {
            const int e = kp[k0 + z];
            const cplx v = at(e >> 16, e & 0xffff);
            ar += v.x; ai += v.y;
        }
        for (int z = lane; z < np; z += 64) {
            const int e = pm[p0 + z];
            const cplx v = at(e >> 16, e & 0xffff);
            br += v.x; bi += v.y;
        }
        // pair z = ia * np + ib, z = lane, lane + 64, ...: (ia, ib) advance by (64 / np, 64 % np) with one carry
        const int dq = 64 / np, dr = 64 - dq * np;
        int ia = lane / np, ib = lane - ia * np;
        while (ia < nk) {
            const int ea = kp[k0 + ia], eb = pm[p0 + ib];
            const cplx g1 = at(eb >> 16, ea & 0xffff), g2 = at(ea >> 16, eb & 0xffff);
            cr += g1.x * g2.x - g1.y * g2.y;
            ci += g1.x * g2.y + g1.y * g2.x;
            ia += dq; ib += dr;
            if (ib >= np) { ib -= np; ++ia; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            ar += __shfl_xor(ar, off); ai += __shfl_xor(ai, off);
            br += __shfl_xor(br, off); bi += __shfl_xor(bi, off);
            cr += __shfl_xor(cr, off); ci += __shfl_xor(ci, off);
        }
        if (lane == 0) { out[3 * q] = cmake(ar, ai); out[3 * q + 1] = cmake(br, bi); out[3 * q + 2] = cmake(cr, ci); }
    }
    // short and empty lists: a thread per momentum transfer
    for (int j = nlong + tid; j < nq; j += (int)blockDim.x) {
        const int q = order[j];
        const int k0 = koff[q], nk = koff[q + 1] - k0, p0 = poff[q], np = poff[q + 1] - p0;
        double ar = 0, ai = 0, br = 0, bi = 0, cr = 0, ci = 0;
        for (int z = 0; z < nk; ++z) {
            const int e = kp[k0 + z];
            const cplx v = at(e >> 16, e & 0xffff);
            ar += v.x; ai += v.y;
        }
        for (int z = 0; z < np; ++z) {
            const int e = pm[p0 + z];
            const cplx v = at(e >> 16, e & 0xffff);
            br += v.x; bi += v.y;
        }
        for (int ia = 0; ia < nk; ++ia) {
            const int ea = kp[k0 + ia];
            for (int ib = 0; ib < np; ++ib) {
                const int eb = pm[p0 + ib];
                const cplx g1 = at(eb >> 16, ea & 0xffff), g2 = at(ea >> 16, eb & 0xffff);
                cr += g1.x * g2.x - g1.y * g2.y;
                ci += g1.x * g2.y + g1.y * g2.x;
            }
        }
        out[3 * q] = cmake(ar, ai); out[3 * q + 1] = cmake(br, bi); out[3 * q + 2] = cmake(cr, ci);
    }
}

// the block's sum of v[0..NV), the same on every thread: wave shuffles, then the per-wave partials in wave order
template <int NV>
__device__ inline void sf_block_sum(double (&v)[NV], double (*red)[NV]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k)
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off);
    if (lane == 0)
        for (int k = 0; k < NV; ++k) red[wave][k] = v[k];
    __syncthreads();
    for (int k = 0; k < NV; ++k) {
        double t = 0.0;
        for (int i = 0; i < nwave; ++i) t += red[i][k];
        v[k] = t;
    }
}

__global__ __launch_bounds__(256) void ueg_pair_finish_kernel(const cplx *G, const cplx *part, int M, int nq,
                                                              const double *vqvec, double vol, const double *H1diag,
                                                              cplx *E, cplx *two) {
    __shared__ double red[4][4];
    const int g = blockIdx.x, tid = threadIdx.x;
    const cplx *Gg = G + (long)g * 2 * M * M;
    const cplx *pa = part + (long)g * 2 * nq * 3, *pb = pa + (long)nq * 3;
    cplx *tw = two + (long)g * 4 * nq;
    double v[4] = {0, 0, 0, 0};                            // ke, pe (re, im)
    for (int e = tid; e < 2 * M; e += 256) {
        const int s = e / M, i = e - s * M;
        const cplx x = Gg[((long)s * M + i) * M + i];
        v[0] += H1diag[e] * x.x; v[1] += H1diag[e] * x.y;
    }
    for (int q = tid; q < nq; q += 256) {
        const cplx ka = pa[3 * q], qa = pa[3 * q + 1], xa = pa[3 * q + 2];
        const cplx kb = pb[3 * q], qb = pb[3 * q + 1], xb = pb[3 * q + 2];
        const cplx taa = csub(cmul(ka, qa), xa), tbb = csub(cmul(kb, qb), xb), tab = cmul(ka, qb), tba = cmul(kb, qa);
        tw[q] = taa; tw[nq + q] = tab; tw[2 * nq + q] = tba; tw[3 * nq + q] = tbb;
        const double f = vqvec[q] / (2.0 * vol);
        v[2] += f * (taa.x + tbb.x + tab.x + tba.x);
        v[3] += f * (taa.y + tbb.y + tab.y + tba.y);
    }
    sf_block_sum<4>(v, red);
    if (tid == 0) {
        E[3 * g] = cmake(v[0] + v[2], v[1] + v[3]);
        E[3 * g + 1] = cmake(v[0], v[1]);
        E[3 * g + 2] = cmake(v[2], v[3]);
    }
}

// out_c[e] = sum_g wt[g] two[g][e] (complex weights wt_c, or real ones wt_r), acc_r[e] += its real part; Green's
// functions of weight zero are left out whatever they hold
__global__ void ueg_sf_wsum_kernel(const cplx *two, const cplx *wt_c, const double *wt_r, int n, long len, cplx *out_c,
                                   double *acc_r) {
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (e >= len) return;
    cplx acc = cmake(0.0, 0.0);
    for (int g = 0; g < n; ++g) {
        const cplx wt = wt_c ? wt_c[g] : cmake(wt_r[g], 0.0);
        if (wt.x == 0.0 && wt.y == 0.0) continue;
        cfma(acc, wt, two[(long)g * len + e]);
    }
    if (out_c) out_c[e] = acc;
    if (acc_r) acc_r[e] += acc.x;
}

// ke = sum_s sum_ij T_s[i,j] G_s[i,j], pe = U sum_i G_a[i,i] G_b[i,i]; one work-group per Green's function
__global__ __launch_bounds__(256) void hubbard_energy_full_g_kernel(const cplx *G, const cplx *T, double U, int M, cplx *E) {
    __shared__ double red[4][4];
    const int g = blockIdx.x, tid = threadIdx.x;
    const cplx *Gg = G + (long)g * 2 * M * M;
    double v[4] = {0, 0, 0, 0};
    for (long e = tid; e < 2L * M * M; e += 256) {
        const cplx t = T[e], x = Gg[e];
        v[0] += t.x * x.x - t.y * x.y; v[1] += t.x * x.y + t.y * x.x;
    }
    for (int i = tid; i < M; i += 256) {
        const cplx a = Gg[(long)i * M + i], b = Gg[(long)M * M + (long)i * M + i];
        v[2] += U * (a.x * b.x - a.y * b.y); v[3] += U * (a.x * b.y + a.y * b.x);
    }
    sf_block_sum<4>(v, red);
    if (tid == 0) {
        E[3 * g] = cmake(v[0] + v[2], v[1] + v[3]);
        E[3 * g + 1] = cmake(v[0], v[1]);
        E[3 * g + 2] = cmake(v[2], v[3]);
    }
}

}  // namespace

int k_ueg_pair_mode(afq_handle *h) {
    const size_t P = (size_t)h->M | 1;
    if (sizeof(cplx) * h->M * P <= SF_LDS_MAX) return 0;
    if (sizeof(cplx) * h->ueg_nrows * P <= SF_LDS_MAX) return 1;
    return 2;
}

int k_ueg_pair_sums(afq_handle *h, const cplx *G, int n, cplx *E, cplx *two) {
    if (!h->sf_kp) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "UEG pair sums: the packed index lists need M < 65536");
    const int M = h->M, nq = h->nq, mode = k_ueg_pair_mode(h);
    int rc = dev_grow(h, LT_SYSTEM, &h->sf_ws, &h->sf_ws_len, (size_t)n * 2 * nq * 3, "UEG pair sums");
    if (rc) return rc;
    const int P = mode == 2 ? M : (M | 1);
    const size_t lds = mode == 0 ? sizeof(cplx) * M * P : mode == 1 ? sizeof(cplx) * h->ueg_nrows * P : 0;
    const dim3 grid(2 * n), block(SF_THREADS);
    if (mode == 0) {
        static size_t lds_set[AFQ_MAX_DEVICES] = {0};
        AFQ_HIP(h, afq_raise_lds((const void *)ueg_pair_kernel<0>, lds, lds_set));
        AFQ_LAUNCH(h, ueg_pair_kernel<0>, grid, block, lds, h->stream, G, h->sf_ws, M, nq, P, h->ueg_koff, h->sf_kp,
                   h->ueg_poff, h->sf_pm, h->ueg_rows, h->ueg_nrows, h->sf_order, h->sf_nlong);
    } else if (mode == 1) {
        static size_t lds_set[AFQ_MAX_DEVICES] = {0};
        AFQ_HIP(h, afq_raise_lds((const void *)ueg_pair_kernel<1>, lds, lds_set));
        AFQ_LAUNCH(h, ueg_pair_kernel<1>, grid, block, lds, h->stream, G, h->sf_ws, M, nq, P, h->ueg_koff, h->ueg_kp,
                   h->ueg_poff, h->ueg_pm, h->ueg_rows, h->ueg_nrows, h->sf_order, h->sf_nlong);
    } else {
        AFQ_LAUNCH(h, ueg_pair_kernel<2>, grid, block, 0, h->stream, G, h->sf_ws, M, nq, P, h->ueg_koff, h->sf_kp,
                   h->ueg_poff, h->sf_pm, h->ueg_rows, h->ueg_nrows, h->sf_order, h->sf_nlong);
    }
    AFQ_POST(h);
    AFQ_LAUNCH(h, ueg_pair_finish_kernel, dim3(n), dim3(256), 0, h->stream, G, h->sf_ws, M, nq, h->vqvec, h->vol,
               h->H1diag, E, two);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_ueg_sf_two(afq_handle *h, int n, cplx **two, cplx **E) {
    const size_t nt = (size_t)n * 4 * h->nq;
    int rc = dev_grow(h, LT_SYSTEM, &h->sf_two, &h->sf_two_len, nt + (size_t)3 * n, "UEG pair sums");
    *two = h->sf_two;
    *E = h->sf_two ? h->sf_two + nt : nullptr;
    return rc;
}

int k_ueg_sf_wsum(afq_handle *h, const cplx *two, int n, const cplx *wt_c, const double *wt_r, cplx *out_c, double *acc_r) {
    const long len = 4L * h->nq;
    AFQ_LAUNCH(h, ueg_sf_wsum_kernel, dim3((unsigned)((len + 127) / 128)), dim3(128), 0, h->stream, two, wt_c, wt_r, n,
               len, out_c, acc_r);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_energy_hubbard_full_g(afq_handle *h, const cplx *G, int n, cplx *E) {
    AFQ_LAUNCH(h, hubbard_energy_full_g_kernel, dim3(n), dim3(256), 0, h->stream, G, h->H1, h->U, h->M, E);
    AFQ_POST(h);
    return AFQ_OK;
}
