// Density and spin correlation functions of full Green's functions G [2, M, M] (spin 0 = up, 1 = down), by Wick's
// theorem for one pair of determinants: corr [5, M, M],
//   corr[2s+t][i,j] = G_s[i,i] G_t[j,j]                                    s != t   <n_is n_jt>
//   corr[2s+s][i,j] = G_s[i,i] G_s[j,j] + G_s[i,j] (d_ij - G_s[j,i])                <n_is n_js>
//   corr[4][i,j]    = G_0[i,j] (d_ij - G_1[j,i])                                    <S+_i S-_j>
// (slices 0-3 are the same for G[i,j] = <c+_i c_j> and for its transpose; slice 4 is transposed with G).
//
// corr_tile_kernel: one work-group per (output tile (I, J) of CT x CT elements, chunk of WCH Green's functions).  Per
// Green's function and spin it needs the tile G[I, J], the tile G[J, I] transposed and the diagonal entries of the rows
// of I and of J.  Both tiles are read with coalesced 16-byte loads along their rows (a wave reads two whole 512-byte tile
// rows per instruction).  G[I, J] stays in registers; G[J, I] goes to LDS as it was read and comes back transposed: the
// pitch of CT + 1 elements (16 bytes each) puts the 16 lanes a ds_read_b128 group serves on 16 different 16-byte slots
// ((33 c + r) mod 16 = (c + r) mod 16, and every group holds 16 values of c that differ mod 16), and the row-wise
// ds_write_b128 is contiguous.  The diagonals come from corr_diag_kernel's [n, 2, M] copy (read strided once, not once
// per tile) through LDS.  The loads of the next Green's function are issued before the arithmetic of the current one.
// The five accumulators of a thread's four elements stay in registers over the chunk.
//
// Reproducibility: no atomics.  A chunk is WCH Green's functions whatever the device (a compile-time constant, not a
// function of the CU count or of free memory), summed in index order; more than one chunk leaves partial sums
// [nchunk, 5, M, M] that corr_combine_kernel adds in chunk order.  Same input, same bits.
// k_corr_full_g is the same kernel with chunks of one Green's function and no weights: its "partial sums" are the result.
#include "afq_internal.h"

namespace {

constexpr int CT = 32;              // tile edge (tests/test_gpu_corr.py takes its sizes from it)
constexpr int CP = CT + 1;          // LDS pitch of the transposed tile
constexpr int CTHREADS = 256;       // 8 rows of 32 lanes: a thread holds rows r0, r0 + 8, r0 + 16, r0 + 24 of its column
constexpr int CROWS = CT * CT / CTHREADS;
constexpr int CORR_WCH = 32;        // Green's functions per chunk of the weighted sum

__global__ void corr_diag_kernel(const cplx *G, cplx *diag, int M, long total) {
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;         // e = (g * 2 + s) * M + i
    if (e >= total) return;
    const long gs = e / M, i = e - gs * M;
    diag[e] = G[(gs * M + i) * M + i];
}

struct CorrLoad {
    cplx a[2][CROWS], b[2][CROWS], d;
};

// the operands of Green's function g for this thread: its elements of G_s[I, J] and of G_s[J, I] (zero outside the
// matrix), and for the first 4 CT threads one diagonal entry (s, I or J, k) each
__device__ inline void corr_load(CorrLoad &L, const cplx *G, const cplx *diag, long g, int M, int I0, int J0) {
    const int tid = threadIdx.x, c = tid & (CT - 1), r0 = tid >> 5;
    const cplx zero = cmake(0.0, 0.0);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const cplx *Gs = G + (g * 2 + s) * (long)M * M;
#pragma unroll
        for (int k = 0; k < CROWS; ++k) {
            const int r = r0 + 8 * k;
            L.a[s][k] = L.b[s][k] = zero;
            if (I0 + r < M && J0 + c < M) L.a[s][k] = Gs[(long)(I0 + r) * M + J0 + c];
            if (J0 + r < M && I0 + c < M) L.b[s][k] = Gs[(long)(J0 + r) * M + I0 + c];
        }
    }
    L.d = zero;
    if (tid < 4 * CT) {
        const int s = tid >> 6, i = ((tid >> 5) & 1 ? J0 : I0) + c;
        if (i < M) L.d = diag[(g * 2 + s) * (long)M + i];
    }
}

template <bool WEIGHTED>      // (two waves per SIMD: two work-groups per CU keep 128 KiB of loads in flight)
__global__ __launch_bounds__(CTHREADS, 2) void corr_tile_kernel(const cplx *G, const cplx *diag, const cplx *wt, int n, int M,
                                                             int nt, cplx *part) {
    __shared__ __align__(16) cplx Bt[2][CT * CP];          // G_s[J, I] as read: Bt[s][r * CP + c] = G_s[J0 + r, I0 + c]
    __shared__ __align__(16) cplx dg[2][2][CT];            // dg[s][0][k] = G_s[I0 + k, I0 + k], dg[s][1][k] the same of J
    constexpr int WCH = WEIGHTED ? CORR_WCH : 1;
    const int tid = threadIdx.x, c = tid & (CT - 1), r0 = tid >> 5;
    const int ntile = nt * nt;
    const long chunk = blockIdx.x / ntile;
    const int tile = (int)(blockIdx.x - chunk * ntile);
    const int I0 = (tile / nt) * CT, J0 = (tile % nt) * CT;
    const long gend = (chunk + 1) * WCH < n ? (chunk + 1) * WCH : n;
    // the Green's functions of weight zero are left out whatever they hold
    auto next = [&](long g) {
        if constexpr (WEIGHTED) while (g < gend && wt[g].x == 0.0 && wt[g].y == 0.0) ++g;
        return g;
    };
    cplx acc[5][CROWS];
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
        for (int k = 0; k < CROWS; ++k) acc[q][k] = cmake(0.0, 0.0);
    CorrLoad L;
    long g = next(chunk * WCH);
    if (g < gend) corr_load(L, G, diag, g, M, I0, J0);
    while (g < gend) {
        cplx a[2][CROWS];
        __syncthreads();                                    // the previous Green's function has been read out of LDS
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int k = 0; k < CROWS; ++k) {
                a[s][k] = L.a[s][k];
                Bt[s][(r0 + 8 * k) * CP + c] = L.b[s][k];
            }
        if (tid < 4 * CT) dg[tid >> 6][(tid >> 5) & 1][c] = L.d;
        __syncthreads();
        cplx w = cmake(1.0, 0.0);
        if constexpr (WEIGHTED) w = wt[g];
        g = next(g + 1);
        if (g < gend) corr_load(L, G, diag, g, M, I0, J0);  // in flight during the arithmetic below
        const cplx dj0 = dg[0][1][c], dj1 = dg[1][1][c];
#pragma unroll
        for (int k = 0; k < CROWS; ++k) {
            const int r = r0 + 8 * k;
            const double dlt = (I0 + r == J0 + c) ? 1.0 : 0.0;
            const cplx di0 = dg[0][0][r], di1 = dg[1][0][r];
            const cplx t0 = Bt[0][c * CP + r], t1 = Bt[1][c * CP + r];          // G_s[j, i]
            const cplx m0 = cmake(dlt - t0.x, -t0.y), m1 = cmake(dlt - t1.x, -t1.y);
            cplx v[5];
            v[0] = cmul(di0, dj0); cfma(v[0], a[0][k], m0);
            v[1] = cmul(di0, dj1);
            v[2] = cmul(di1, dj0);
            v[3] = cmul(di1, dj1); cfma(v[3], a[1][k], m1);
            v[4] = cmul(a[0][k], m1);
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                if constexpr (WEIGHTED) cfma(acc[q][k], w, v[q]);
                else acc[q][k] = v[q];
            }
        }
    }
    const size_t mm = (size_t)M * M;
    cplx *out = part + (size_t)chunk * 5 * mm;
    if (J0 + c < M) {
#pragma unroll
        for (int k = 0; k < CROWS; ++k) {
            const int i = I0 + r0 + 8 * k;
            if (i < M) {
#pragma unroll
                for (int q = 0; q < 5; ++q) out[q * mm + (size_t)i * M + J0 + c] = acc[q][k];
            }
        }
    }
}

// out[e] = sum_c part[c][e], chunks in index order
__global__ void corr_combine_kernel(const cplx *part, int nchunk, size_t len, cplx *out) {
    const size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (e >= len) return;
    cplx acc = part[e];
    for (int ch = 1; ch < nchunk; ++ch) acc = cadd(acc, part[(size_t)ch * len + e]);
    out[e] = acc;
}

// the diagonals of n Green's functions into the head of the handle's scratch, `extra` elements behind them
int corr_prepare(afq_handle *h, const cplx *G, int n, size_t extra, cplx **diag, cplx **rest) {
    const size_t nd = (size_t)n * 2 * h->M;
    int rc = dev_grow(h, LT_SYSTEM, &h->corr_ws, &h->corr_ws_len, nd + extra, "correlation functions");
    if (rc) return rc;
    *diag = h->corr_ws; *rest = h->corr_ws + nd;
    AFQ_LAUNCH(h, corr_diag_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, h->stream, G, h->corr_ws, h->M, (long)nd);
    AFQ_POST(h);
    return AFQ_OK;
}

}  // namespace

int k_sum_chunks(afq_handle *h, const cplx *part, int nchunk, size_t len, cplx *out) {
    AFQ_LAUNCH(h, corr_combine_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, h->stream, part, nchunk, len, out);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_corr_full_g(afq_handle *h, const cplx *G, int n, cplx *out) {
    const int M = h->M, nt = (M + CT - 1) / CT;
    if ((size_t)nt * nt * n > 0x7fffffffu) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "correlation functions: more than 2^31 tiles in one call");
    cplx *diag, *rest;
    int rc = corr_prepare(h, G, n, 0, &diag, &rest);
    if (rc) return rc;
    AFQ_LAUNCH(h, corr_tile_kernel<false>, dim3((unsigned)(nt * nt * n)), dim3(CTHREADS), 0, h->stream, G, diag,
               (const cplx *)nullptr, n, M, nt, out);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_corr_wsum(afq_handle *h, const cplx *G, int n, const cplx *wt_c, cplx *out) {
    const int M = h->M, nt = (M + CT - 1) / CT, nchunk = (n + CORR_WCH - 1) / CORR_WCH;
    const size_t len = (size_t)5 * M * M;
    if ((size_t)nt * nt * nchunk > 0x7fffffffu) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "correlation functions: more than 2^31 tiles in one call");
    cplx *diag, *part;
    int rc = corr_prepare(h, G, n, nchunk > 1 ? nchunk * len : 0, &diag, &part);
    if (rc) return rc;
    AFQ_LAUNCH(h, corr_tile_kernel<true>, dim3((unsigned)(nt * nt * nchunk)), dim3(CTHREADS), 0, h->stream, G,
               diag, wt_c, n, M, nt, nchunk > 1 ? part : out);
    AFQ_POST(h);
    return nchunk > 1 ? k_sum_chunks(h, part, nchunk, len, out) : AFQ_OK;
}
