// Pair-field correlation functions of full Green's functions G [2, M, M] (spin 0 = up, 1 = down) over a bond table
// nbr int32 [nb, M] (nbr[b][i] = the partner site of i along bond b, -1 = none), by Wick's theorem for one pair of
// determinants.  With D+(k, l) = c+_k,up c+_l,down and G[i,j] = <c+_i c_j>,
//   pair[b, b', i, j] = <D+(i, nbr[b][i]) D(j, nbr[b'][j])> = G_0[i, j] G_1[nbr[b][i], nbr[b'][j]]     [nb, nb, M, M]
// and 0 where either partner is -1 (opposite spins: no exchange term).  For the transposed convention (the
// back-propagated G is the transpose) the same array is the correlator with both index pairs exchanged: the element
// [b, b', i, j] then holds <D+(j, nbr[b'][j]) D(i, nbr[b][i])>, i.e. pair[b', b, j, i] of the definition above.
//
// pair_tile_kernel: one work-group of PT x PT threads per (output tile (I, J), block of PB x PB bond pairs, chunk of
// PAIR_WCH Green's functions); up to PB bonds (the lattice's on-site, +-x, +-y) there is one block and the tile's G_0
// elements are read once for all (b, b').  A thread owns one element (i, j), lanes along j: the G_0 load and the nb^2
// stores are 16-byte accesses to contiguous runs of PT elements, and so are the gathers G_1[nbr[b][i], nbr[b'][J]] where
// nbr[b'] maps the tile's columns to runs (a periodic lattice: one or two runs per tile row); nothing relies on that, an
// arbitrary table only coalesces worse.  No LDS: what the PB^2 gathers of a tile touch (at most PB PT rows by PB PT
// columns of G_1) is served by the caches.  A partner of -1 (and every lane outside the matrix, and every bond past nb)
// reads element 0 of the matrix and discards it by a select, so that the loads are issued without branches and nothing
// such a lane reads (a NaN included) reaches a sum.  The PB^2 accumulators stay in registers over the chunk.
//
// Reproducibility: as k_corr.hip.  No atomics; a chunk is PAIR_WCH Green's functions whatever the device, summed in
// index order (weight-zero ones left out whatever they hold); more than one chunk leaves partial sums
// [nchunk, nb, nb, M, M] in the handle's scratch that k_sum_chunks (k_corr.hip) adds in chunk order.  Same input, same bits.
// k_pair_full_g is the same kernel with chunks of one Green's function and no weights.
#include "afq_internal.h"

namespace {

constexpr int PT = 16;              // tile edge (tests/test_gpu_pair.py takes its sizes from it)
constexpr int PTHREADS = PT * PT;   // one element per thread: a wave holds four rows of 16 lanes
constexpr int PB = 5;               // bonds per block on either side: PB^2 complex accumulators per thread
constexpr int PAIR_WCH = 64;        // Green's functions per chunk of the weighted sum

template <bool WEIGHTED>
__global__ __launch_bounds__(PTHREADS) void pair_tile_kernel(const cplx *G, const int *nbr, const cplx *wt, int n, int M,
                                                            int nb, int nt, int nblk, cplx *part) {
    constexpr int WCH = WEIGHTED ? PAIR_WCH : 1;
    const int tid = threadIdx.x, c = tid & (PT - 1), r = tid / PT;
    const unsigned ntile = (unsigned)nt * nt, nbb = (unsigned)nblk * nblk;
    unsigned rest = blockIdx.x;                                 // (chunk, bond block, tile), the tile fastest
    const int tile = (int)(rest % ntile); rest /= ntile;
    const int blk = (int)(rest % nbb);
    const long chunk = rest / nbb;
    const int i = (tile / nt) * PT + r, j = (tile % nt) * PT + c;
    const int b0 = (blk / nblk) * PB, c0 = (blk % nblk) * PB;
    const bool in = i < M && j < M;
    const size_t mm = (size_t)M * M;
    // the partners of this thread's i along the block's bonds b and of its j along the bonds b'
    size_t ri[PB];
    int cj[PB];
    bool oki[PB], okj[PB];
#pragma unroll
    for (int k = 0; k < PB; ++k) {
        const int pi = in && b0 + k < nb ? nbr[(size_t)(b0 + k) * M + i] : -1;
        const int pj = in && c0 + k < nb ? nbr[(size_t)(c0 + k) * M + j] : -1;
        oki[k] = pi >= 0; okj[k] = pj >= 0;
        ri[k] = oki[k] ? (size_t)pi * M : 0;
        cj[k] = okj[k] ? pj : 0;
    }
    const long gend = (chunk + 1) * WCH < n ? (chunk + 1) * WCH : n;
    // the Green's functions of weight zero are left out whatever they hold
    auto next = [&](long g) {
        if constexpr (WEIGHTED) while (g < gend && wt[g].x == 0.0 && wt[g].y == 0.0) ++g;
        return g;
    };
    const cplx zero = cmake(0.0, 0.0);
    cplx acc[PB][PB];
#pragma unroll
    for (int k = 0; k < PB; ++k)
#pragma unroll
        for (int l = 0; l < PB; ++l) acc[k][l] = zero;
    for (long g = next(chunk * WCH); g < gend; g = next(g + 1)) {
        const cplx *G0 = G + (size_t)g * 2 * mm, *G1 = G0 + mm;
        cplx a = in ? G0[(size_t)i * M + j] : zero;
        if constexpr (WEIGHTED) a = cmul(wt[g], a);
        cplx g1[PB][PB];
#pragma unroll
        for (int k = 0; k < PB; ++k)
#pragma unroll
            for (int l = 0; l < PB; ++l) g1[k][l] = G1[ri[k] + cj[l]];
#pragma unroll
        for (int k = 0; k < PB; ++k)
#pragma unroll
            for (int l = 0; l < PB; ++l) {
                const cplx v = oki[k] && okj[l] ? g1[k][l] : zero;
                if constexpr (WEIGHTED) cfma(acc[k][l], a, v);
                else acc[k][l] = cmul(a, v);
            }
    }
    if (!in) return;
    cplx *out = part + (size_t)chunk * nb * nb * mm + (size_t)i * M + j;
#pragma unroll
    for (int k = 0; k < PB; ++k)
#pragma unroll
        for (int l = 0; l < PB; ++l)
            if (b0 + k < nb && c0 + l < nb) out[((size_t)(b0 + k) * nb + c0 + l) * mm] = acc[k][l];
}

// the grid of nchunk chunks: tiles per edge, bond blocks per side, work-groups (0: more than 2^31 - 1)
unsigned pair_grid(const afq_handle *h, int nchunk, int *nt, int *nblk) {
    *nt = (h->M + PT - 1) / PT; *nblk = (h->pair_nb + PB - 1) / PB;
    const size_t per = (size_t)*nt * *nt * *nblk * *nblk;               // (nt < 2^27 and nblk <= 4: no overflow)
    return per * (size_t)nchunk > 0x7fffffffu ? 0u : (unsigned)(per * nchunk);
}

}  // namespace

int k_pair_full_g(afq_handle *h, const cplx *G, int n, cplx *out) {
    int nt, nblk;
    const unsigned grid = pair_grid(h, n, &nt, &nblk);
    if (!grid) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "pairing correlations: more than 2^31 tiles in one call");
    AFQ_LAUNCH(h, pair_tile_kernel<false>, dim3(grid), dim3(PTHREADS), 0, h->stream, G, (const int *)h->pair_nbr,
               (const cplx *)nullptr, n, h->M, h->pair_nb, nt, nblk, out);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_pair_wsum(afq_handle *h, const cplx *G, int n, const cplx *wt_c, cplx *out) {
    const int nchunk = (n + PAIR_WCH - 1) / PAIR_WCH;
    const size_t len = (size_t)h->pair_nb * h->pair_nb * h->M * h->M;
    int nt, nblk;
    const unsigned grid = pair_grid(h, nchunk, &nt, &nblk);
    if (!grid) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "pairing correlations: more than 2^31 tiles in one call");
    if (nchunk > 1) AFQ_TRY(dev_grow(h, LT_SYSTEM, &h->pair_ws, &h->pair_ws_len, nchunk * len, "pairing correlations"));
    AFQ_LAUNCH(h, pair_tile_kernel<true>, dim3(grid), dim3(PTHREADS), 0, h->stream, G, (const int *)h->pair_nbr, wt_c, n,
               h->M, h->pair_nb, nt, nblk, nchunk > 1 ? h->pair_ws : out);
    AFQ_POST(h);
    return nchunk > 1 ? k_sum_chunks(h, h->pair_ws, nchunk, len, out) : AFQ_OK;
}
