// Finite-temperature AFQMC walkers of the Hubbard model with discrete Hirsch fields (thermal_propagation/hubbard.py,
// walkers/thermal.py, walkers/stack.py of the reference; constrained path, spin decomposition: every matrix is real).
//
// A thermal walker has no Slater determinant: it carries G_s = [I + B_L .. B_1]^-1 per spin, f64 [2, M, M], and a stack
// of nbins products of stack_size propagators each, f64 [nbins, 2, M, M].  The slice counter, the block and the in-bin
// counter are the same for every walker and live on the handle; the driver moves the population through the slices
// together.  M <= 64: a walker's working set stays in LDS.  A handle configured with AFQ_THERMAL_DELAYED takes the second
// route below (th_engine WIDE: th_launch_greens<double> and the slice launch read it) and reaches M = 128 =
// afq_thermal_delayed_max_basis().  Every kernel with dynamic LDS is launched by th_launch (thermal_strat.h).
//
//   thermal_greens_kernel   G of every (walker, spin) from the stack: thermal_strat.h's engine with T = double.
//   thermal_slice_kernel    one work-group per walker, both spins' G in LDS: the M single-site updates of
//                           propagate_walker_constrained, then B_s = diag(BV_s) BH1_s onto the walker's current bin.
//   thermal_wrap_kernel     G_s <- BT_s G_s BT_s^-1 (two MFMA products) per (walker, spin).
// With AFQ_THERMAL_DELAYED
//   thermal_greens_wide_kernel    thermal_wide.h's engine with T = double: one real matrix in LDS, two columns per lane.
//   thermal_slice_delayed_kernel  the same M single-site updates as the delayed (blocked) updates of determinant QMC:
//                           G of both spins stays in device memory; per panel of TD_KB sites the panel's columns and rows
//                           are loaded into LDS and kept current site by site, the rank-1 factors accumulate as
//                           U [M, KB] and W [KB, M], and G <- G + U W closes the panel as one fp64 MFMA product.
// and, for every kind of thermal handle, afq_thermal_estimates: the mixed estimator's sums (estimators/mixed.py:180-233)
//   thermal_sweep_reduce_kernel   every walker's (E, T, V, nav) over the bins of the sweep, added in bin order.
//   thermal_one_rdm_kernel        sum_w weight_w Re G_w.
#include "thermal_wide.h"
#include <cstring>

#define TH_MAXM 64
#define TD_KB 16                // sites per panel of the delayed updates (a multiple of the MFMA's k = 4)
#define TD_CP (TD_KB + 1)       // pitch of the [M, TD_KB] panels in LDS: a column read walks the banks

namespace {

inline size_t th_slice_lds(int M) { return sizeof(double) * (3 * ts_mat(M) + 6 * 64); }
inline size_t th_wrap_lds(int M) { return sizeof(double) * ts_mat(M); }
// LDS of the delayed slice kernel: bv [2][128]; per spin the panel's columns and U [M, TD_KB] (pitch TD_CP), its rows and
// W [TD_KB, M | 1]; behind the sites the same room holds the one matrix of the stack update
inline size_t td_panel_scalars(int M) { return 2 * (2 * (size_t)M * TD_CP + 2 * (size_t)TD_KB * (M | 1)); }
inline size_t th_slice_delayed_lds(int M) {
    const size_t p = td_panel_scalars(M), x = ts_mat(M);
    return sizeof(double) * (2 * TW_COLS + (p > x ? p : x));
}

struct ThSliceArgs {
    double *G, *stack, *weight;
    const double *u, *BH1;
    int *fields;
    int M, nbins, block, counter;
    double delta[2][2], auxf[2][2], exp_eshift;
};

__global__ __launch_bounds__(TH_THREADS) void thermal_slice_kernel(ThSliceArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int M = a.M, LD = M | 1, tid = threadIdx.x, w = blockIdx.x;
    const size_t mat = ts_mat(M);
    double *Gs = (double *)smem;                       // [2][mat]
    double *X = Gs + 2 * mat;
    double *colv = X + mat, *rowv = colv + 128, *bv = rowv + 128;    // [2][64] each
    const long mm = (long)M * M;
    double *Gw = a.G + (long)w * 2 * mm;
    for (int e = tid; e < 2 * M * M; e += TH_THREADS) {
        const int s = e / (M * M), r = (e / M) % M, c = e % M;
        Gs[s * mat + r * LD + c] = Gw[e];
    }
    __syncthreads();
    double wt = a.weight[w];
    for (int i = 0; i < M; ++i) {
        const double g0 = Gs[i * LD + i], g1 = Gs[mat + i * LD + i];
        double p0 = 0.5 * ((1.0 + (1.0 - g0) * a.delta[0][0]) * (1.0 + (1.0 - g1) * a.delta[0][1]));
        double p1 = 0.5 * ((1.0 + (1.0 - g0) * a.delta[1][0]) * (1.0 + (1.0 - g1) * a.delta[1][1]));
        p0 = p0 > 0.0 ? p0 : 0.0; p1 = p1 > 0.0 ? p1 : 0.0;
        const double norm = p0 + p1;
        const double u = a.u[(long)w * M + i];        // consumed whatever norm is
        if (norm > 0.0) {                             // (the same value in every thread: a uniform branch)
            wt = wt * norm * a.exp_eshift;
            const int x = u < p0 / norm ? 0 : 1;
            if (tid < 128) {
                const int s = tid >> 6, r = tid & 63;
                if (r < M) {
                    colv[s * 64 + r] = Gs[s * mat + r * LD + i];
                    rowv[s * 64 + r] = (r == i ? 1.0 : 0.0) - Gs[s * mat + i * LD + r];
                }
            }
            __syncthreads();
            const double f0 = a.delta[x][0] / (1.0 + (1.0 - g0) * a.delta[x][0]);
            const double f1 = a.delta[x][1] / (1.0 + (1.0 - g1) * a.delta[x][1]);
            for (int e = tid; e < 2 * M * M; e += TH_THREADS) {
                const int s = e / (M * M), r = (e / M) % M, c = e % M;
                double *g = &Gs[s * mat + r * LD + c];
                *g = fma(-(s ? f1 : f0) * colv[s * 64 + r], rowv[s * 64 + c], *g);
            }
            if (tid == 0) {
                bv[i] = a.auxf[x][0]; bv[64 + i] = a.auxf[x][1];
                if (a.fields) a.fields[(long)w * M + i] = x;
            }
            __syncthreads();
        } else {
            wt = 0.0;
            if (tid == 0) {
                bv[i] = a.auxf[0][0]; bv[64 + i] = a.auxf[0][1];
                if (a.fields) a.fields[(long)w * M + i] = -1;
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < 2 * M * M; e += TH_THREADS) {
        const int s = e / (M * M), r = (e / M) % M, c = e % M;
        Gw[e] = Gs[s * mat + r * LD + c];
    }
    if (tid == 0) a.weight[w] = wt;
    // stack[block, s] = diag(BV_s) BH1_s (counter == 0 ? I : stack[block, s])
    for (int s = 0; s < 2; ++s) {
        double *S = a.stack + (((long)w * a.nbins + a.block) * 2 + s) * mm;
        const double *BH = a.BH1 + s * mm, *b = bv + s * 64;
        if (a.counter == 0) {
            for (int e = tid; e < M * M; e += TH_THREADS) S[e] = b[e / M] * BH[e];
        } else {
            ts_gemm<double>(M, [&](int r, int k) { return b[r] * BH[r * M + k]; }, [&](int k, int c) { return S[k * M + c]; },
                    [&](int r, int c, double x) { X[r * LD + c] = x; });
            __syncthreads();
            for (int e = tid; e < M * M; e += TH_THREADS) S[e] = X[(e / M) * LD + e % M];
            __syncthreads();
        }
    }
}

// The slice by delayed updates.  Site i = i0 + j of the panel i0 .. i0 + kb - 1 reads the current G_ii of both spins off
// the panel's columns, decides as thermal_slice_kernel does, and leaves u = -f col_i in column j of U and w = e_i - row_i
// in row j of W (zeros for a site whose probabilities both vanish); only the panel's later columns and rows are brought
// up to date, by the fma of the direct kernel, so within a panel every decision sees the direct route's bits.  The
// trailing G <- G + U W runs over G in device memory, 16 x 16 tiles with G's tile as the accumulator's start; rows,
// columns and k beyond M or beyond kb enter as zero operands.  No trip count depends on data, every branch is uniform
// over the work-group, every wave is at every barrier.
__global__ __launch_bounds__(TH_THREADS) void thermal_slice_delayed_kernel(ThSliceArgs a) {
    static_assert(TD_KB % 4 == 0 && TD_KB >= 4, "the trailing update steps k by the MFMA's 4");
    extern __shared__ __align__(16) unsigned char smem[];
    const int M = a.M, LD = M | 1, tid = threadIdx.x, w = blockIdx.x;
    const long mm = (long)M * M;
    double *bv = (double *)smem;                       // [2][128]
    double *Cp = bv + 2 * TW_COLS;                     // [2][M][TD_CP] the panel's columns
    double *Up = Cp + 2 * M * TD_CP;                   // [2][M][TD_CP]
    double *Rp = Up + 2 * M * TD_CP;                   // [2][TD_KB][LD] the panel's rows
    double *Wp = Rp + 2 * TD_KB * LD;                  // [2][TD_KB][LD]
    double *X = Cp;                                    // [M][LD] behind the sites
    double *Gw = a.G + (long)w * 2 * mm;
    const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4, nt = (M + 15) >> 4;
    double wt = a.weight[w];
    for (int i0 = 0; i0 < M; i0 += TD_KB) {
        const int kb = M - i0 < TD_KB ? M - i0 : TD_KB;
        for (int e = tid; e < 2 * M * kb; e += TH_THREADS) {
            const int s = e / (M * kb), r = (e / kb) % M, jj = e % kb;
            Cp[(s * M + r) * TD_CP + jj] = Gw[s * mm + (long)r * M + i0 + jj];
        }
        for (int e = tid; e < 2 * kb * M; e += TH_THREADS) {
            const int s = e / (kb * M), jj = (e / M) % kb, c = e % M;
            Rp[(s * TD_KB + jj) * LD + c] = Gw[s * mm + (long)(i0 + jj) * M + c];
        }
        __syncthreads();
        for (int j = 0; j < kb; ++j) {
            const int i = i0 + j;
            const double g0 = Cp[i * TD_CP + j], g1 = Cp[(M + i) * TD_CP + j];
            double p0 = 0.5 * ((1.0 + (1.0 - g0) * a.delta[0][0]) * (1.0 + (1.0 - g1) * a.delta[0][1]));
            double p1 = 0.5 * ((1.0 + (1.0 - g0) * a.delta[1][0]) * (1.0 + (1.0 - g1) * a.delta[1][1]));
            p0 = p0 > 0.0 ? p0 : 0.0; p1 = p1 > 0.0 ? p1 : 0.0;
            const double norm = p0 + p1;
            const double u = a.u[(long)w * M + i];        // consumed whatever norm is
            const bool live = norm > 0.0;                 // (the same value in every thread: uniform branches)
            int x = 0;
            double f0 = 0.0, f1 = 0.0;
            if (live) {
                wt = wt * norm * a.exp_eshift;
                x = u < p0 / norm ? 0 : 1;
                f0 = a.delta[x][0] / (1.0 + (1.0 - g0) * a.delta[x][0]);
                f1 = a.delta[x][1] / (1.0 + (1.0 - g1) * a.delta[x][1]);
            } else {
                wt = 0.0;
            }
            {
                const int s = tid >> 7, r = tid & 127;
                if (r < M) {
                    Up[(s * M + r) * TD_CP + j] = live ? -(s ? f1 : f0) * Cp[(s * M + r) * TD_CP + j] : 0.0;
                    Wp[(s * TD_KB + j) * LD + r] = live ? (r == i ? 1.0 : 0.0) - Rp[(s * TD_KB + j) * LD + r] : 0.0;
                }
            }
            if (tid == 0) {
                bv[i] = a.auxf[x][0]; bv[TW_COLS + i] = a.auxf[x][1];
                if (a.fields) a.fields[(long)w * M + i] = live ? x : -1;
            }
            __syncthreads();
            if (live) {
                const int nc = kb - j - 1;                // the panel's columns and rows still to come
                for (int e = tid; e < 2 * M * nc; e += TH_THREADS) {
                    const int s = e / (M * nc), r = (e / nc) % M, jj = j + 1 + e % nc;
                    double *g = &Cp[(s * M + r) * TD_CP + jj];
                    *g = fma(Up[(s * M + r) * TD_CP + j], Wp[(s * TD_KB + j) * LD + i0 + jj], *g);
                }
                for (int e = tid; e < 2 * nc * M; e += TH_THREADS) {
                    const int s = e / (nc * M), jj = j + 1 + (e / M) % nc, c = e % M;
                    double *g = &Rp[(s * TD_KB + jj) * LD + c];
                    *g = fma(Up[(s * M + i0 + jj) * TD_CP + j], Wp[(s * TD_KB + j) * LD + c], *g);
                }
            }
            __syncthreads();
        }
        // G <- G + U W
        for (int tile = wave; tile < 2 * nt * nt; tile += TH_THREADS / 64) {
            const int s = tile / (nt * nt), t2 = tile % (nt * nt);
            const int row0 = (t2 / nt) << 4, col0 = (t2 % nt) << 4, arow = row0 + lr, bcol = col0 + lr;
            double *Gs = Gw + s * mm;
            d4_t acc;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + lk + 4 * r;
                acc[r] = (row < M && bcol < M) ? Gs[(long)row * M + bcol] : 0.0;
            }
#pragma unroll
            for (int k0 = 0; k0 < TD_KB; k0 += 4) {
                const int k = k0 + lk;
                const double ua = (arow < M && k < kb) ? Up[(s * M + arow) * TD_CP + k] : 0.0;
                const double wb = (bcol < M && k < kb) ? Wp[(s * TD_KB + k) * LD + bcol] : 0.0;
                acc = mfma16(ua, wb, acc);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + lk + 4 * r;
                if (row < M && bcol < M) Gs[(long)row * M + bcol] = acc[r];
            }
        }
        __syncthreads();
    }
    if (tid == 0) a.weight[w] = wt;
    // stack[block, s] = diag(BV_s) BH1_s (counter == 0 ? I : stack[block, s]); the bin is read whole before it is written
    for (int s = 0; s < 2; ++s) {
        double *S = a.stack + (((long)w * a.nbins + a.block) * 2 + s) * mm;
        const double *BH = a.BH1 + s * mm, *b = bv + s * TW_COLS;
        if (a.counter == 0) {
            for (int e = tid; e < M * M; e += TH_THREADS) S[e] = b[e / M] * BH[e];
        } else {
            ts_gemm<double>(M, [&](int r, int k) { return b[r] * BH[r * M + k]; }, [&](int k, int c) { return S[k * M + c]; },
                    [&](int r, int c, double x) { X[r * LD + c] = x; });
            __syncthreads();
            for (int e = tid; e < M * M; e += TH_THREADS) S[e] = X[(e / M) * LD + e % M];
            __syncthreads();
        }
    }
}

// G_s <- BT_s G_s BT_s^-1 per (walker, spin)
__global__ __launch_bounds__(TH_THREADS) void thermal_wrap_kernel(double *G, const double *BT, const double *BTinv, int M) {
    extern __shared__ __align__(16) unsigned char smem[];
    double *X = (double *)smem;
    const int LD = M | 1, s = blockIdx.x & 1;
    const long mm = (long)M * M;
    double *Gd = G + (long)blockIdx.x * mm;
    const double *A = BT + s * mm, *Ai = BTinv + s * mm;
    ts_gemm<double>(M, [&](int r, int k) { return A[r * M + k]; }, [&](int k, int c) { return Gd[k * M + c]; },
            [&](int r, int c, double x) { X[r * LD + c] = x; });
    __syncthreads();
    ts_gemm<double>(M, [&](int r, int k) { return X[r * LD + k]; }, [&](int k, int c) { return Ai[k * M + c]; },
            [&](int r, int c, double x) { Gd[r * M + c] = x; });
}

// every walker's bins <- BTpow [2, M, M], G <- G0 [2, M, M], weight <- 1 (unscaled_weight stays: handler.py:424-430)
__global__ void thermal_reset_kernel(double *stack, double *G, double *weight, const double *BTpow,
                                     const double *G0, int nbins, long per, int nw) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const int w = blockIdx.y;
    if (i < per) {
        const double b = BTpow[i];
        for (int n = 0; n < nbins; ++n) stack[((long)w * nbins + n) * per + i] = b;
        G[(long)w * per + i] = G0[i];
    }
    if (i == 0) weight[w] = 1.0;
}

// ---- afq_thermal_estimates: the estimators' sums of a population of thermal walkers

#define TH_SWEEP_BUDGET ((size_t)2 << 30)      // bytes of G, P and T scratch a sweep takes at a time unless told otherwise

// One thread per walker: (E, T, V, nav) of its nbins Green's functions (E c128 [nbins, nw, 3], nav [nbins, nw]) into
// per_bin [nbins, nw, 4], and their sums, added in bin order from zero, into cols [nw, 4].
__global__ void thermal_sweep_reduce_kernel(const cplx *E, const double *nav, int nw, int nbins, double *cols, double *per_bin) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int ts = 0; ts < nbins; ++ts) {
        const long g = (long)ts * nw + w;
        const double v[4] = {E[3 * g].x, E[3 * g + 1].x, E[3 * g + 2].x, nav[g]};
#pragma unroll
        for (int q = 0; q < 4; ++q) { per_bin[4 * g + q] = v[q]; s[q] += v[q]; }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) cols[4 * w + q] = s[q];
}

// out[e] = sum_w weight_w Re G_w[e] over every walker in walker order, one thread per element: no atomics, the same
// bits on every run
template <class T>
__global__ void thermal_one_rdm_kernel(const T *G, const double *weight, int nw, long len, double *out) {
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (e >= len) return;
    double acc = 0.0;
    for (int w = 0; w < nw; ++w) acc += weight[w] * TsScalar<T>::re(G[(long)w * len + e]);
    out[e] = acc;
}

inline size_t th_up256(size_t b) { return (b + 255) & ~(size_t)255; }

// the energies of n Green's functions from their P [n, 2, M, M]: E c128 [n, 3]; *two (UEG) the per-q pair sums
// [n, 2, 2, nq] in the handle's scratch
int th_energy_n(afq_handle *h, const cplx *P, int n, cplx *E, cplx **two) {
    if (h->th_kind != TH_CPLX_DIAG) return k_energy_hubbard_full_g(h, P, n, E);
    cplx *e_unused = nullptr;
    AFQ_TRY(k_ueg_sf_two(h, n, two, &e_unused));
    return k_ueg_pair_sums(h, P, n, E, *two);
}

// the largest M of a delayed handle: what its three kernels' LDS and the 128 columns of two per lane admit
int th_delayed_bound() {
    int m = TW_COLS;
    while (m > 1 && (ts_greens_wide_lds<double>(m) > TH_LDS_MAX || th_slice_delayed_lds(m) > TH_LDS_MAX || th_wrap_lds(m) > TH_LDS_MAX)) --m;
    return m;
}

}  // namespace

int k_thermal_greens(afq_handle *h, int slice_ix) {
    return th_launch_greens<double>(h, h->th_stack, h->th_G, nullptr, ts_first_bin(h, slice_ix), -1, dim3(2 * h->nw));
}

extern "C" {

int afq_thermal_configure(afq_handle *h, int ntime_slices, int stack_size, int nstblz, const double *BT,
                          const double *BT_inv, const double *BH1, const double *auxf, int options) {
    AFQ_API(h, "afq_thermal_configure");
    if (!h) return AFQ_EINVAL;
    h->th_kind = TH_NONE;
    if (!BT || !BT_inv || !BH1 || !auxf) AFQ_FAIL(h, AFQ_EINVAL, "afq_thermal_configure: null operand");
    const ThEntry me = {"afq_thermal_configure: ", AFQ_THERMAL_DELAYED, AFQ_EUNSUPPORTED,
                        "thermal walkers: charge_decomposition is not supported (spin decomposition only)", AFQ_SYS_HUBBARD,
                        "thermal walkers: Hubbard systems only (no Generic / UEG)", "all"};
    AFQ_TRY(th_screen_options(h, me, options));
    const bool delayed = (options & AFQ_THERMAL_DELAYED) != 0;
    if (delayed)
        AFQ_TRY(th_screen_bound(h, "thermal walkers (delayed_updates)", "sites", TW_COLS, true,
                                {{"the wide Green's function (thermal_greens_wide_kernel)", ts_greens_wide_lds<double>, ""},
                                 {"the delayed slice kernel (thermal_slice_delayed_kernel)", th_slice_delayed_lds, ""},
                                 {"the wrap (thermal_wrap_kernel)", th_wrap_lds, ""}}));
    else if (h->M > TH_MAXM)
        AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: M = " + std::to_string(h->M) + " > 64 sites do not fit a work-group's LDS"
                 "; AFQ_THERMAL_DELAYED (delayed_updates) reaches M = " + std::to_string(th_delayed_bound()));
    AFQ_TRY(th_screen_state(h, me, ntime_slices, stack_size, nstblz));
    hipSetDevice(h->device);
    const int M = h->M, nbins = ntime_slices / stack_size;
    const size_t mm = (size_t)M * M, n = h->nw;
    int rc;
    if ((rc = dev_upload(h, LT_WALKERS, &h->th_BT, BT, 2 * mm)) || (rc = dev_upload(h, LT_WALKERS, &h->th_BTinv, BT_inv, 2 * mm)) ||
        (rc = dev_upload(h, LT_WALKERS, &h->th_BH1, BH1, 2 * mm))) return rc;
    // every bin of a fresh path is BT^stack_size, left-multiplied as PropagatorStack.set_all does (stack.py:238-243)
    std::vector<double> pw(2 * mm, 0.0), tmp(mm);
    for (int s = 0; s < 2; ++s) {
        double *p = &pw[s * mm];
        const double *b = BT + s * mm;
        for (int i = 0; i < M; ++i) p[(size_t)i * M + i] = 1.0;
        for (int it = 0; it < stack_size; ++it) {
            for (int i = 0; i < M; ++i)
                for (int j = 0; j < M; ++j) {
                    double acc = 0.0;
                    for (int k = 0; k < M; ++k) acc += b[(size_t)i * M + k] * p[(size_t)k * M + j];
                    tmp[(size_t)i * M + j] = acc;
                }
            memcpy(p, tmp.data(), sizeof(double) * mm);
        }
    }
    if ((rc = dev_upload(h, LT_WALKERS, &h->th_BTpow, pw.data(), 2 * mm))) return rc;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->th_G, 2 * mm * n)) || (rc = dev_alloc(h, LT_WALKERS, &h->th_G0, 2 * mm)) ||
        (rc = dev_alloc(h, LT_WALKERS, &h->th_stack, 2 * mm * n * nbins)) || (rc = dev_alloc(h, LT_WALKERS, &h->th_u, (size_t)M * n)) ||
        (rc = dev_alloc(h, LT_WALKERS, &h->th_fields, (size_t)M * n)) || (rc = dev_alloc(h, LT_WALKERS, &h->th_nav, n))) return rc;
    // the wide Green's function's scratch, four [M, M] per (walker, spin); a handle configured without the bit holds none
    if ((rc = dev_alloc(h, LT_WALKERS, (double **)&h->th_scratch, delayed ? 2 * ts_greens_wide_scratch(M) * n : (size_t)0))) return rc;
    h->th_engine = delayed ? TH_ENGINE_WIDE : TH_ENGINE_RESIDENT;
    if ((rc = ensure_G(h))) return rc;                  // c128 [nw, 2, M, M]: the one-body density matrices of afq_thermal_energy
    for (int f = 0; f < 2; ++f) for (int s = 0; s < 2; ++s) h->th_auxf[f][s] = auxf[2 * f + s];
    h->th_L = ntime_slices; h->th_ss = stack_size; h->th_nbins = nbins; h->th_nstblz = nstblz;
    h->th_kind = TH_REAL;
    return afq_thermal_reset(h);
}

int afq_thermal_delayed_max_basis(void) { return th_delayed_bound(); }

int afq_thermal_device_allocations(afq_handle *h, int64_t *out) {
    if (!h || !out) return AFQ_EINVAL;
    *out = h->mem.allocations;
    return AFQ_OK;
}

int afq_thermal_reset(afq_handle *h) {
    AFQ_API(h, "afq_thermal_reset");
    if (!h) return AFQ_EINVAL;
    AFQ_TRY(th_need(h, false));
    if (th_complex(h)) return k_thermal_c_reset(h, false);
    const int M = h->M, nbins = h->th_nbins;
    const long per = 2L * M * M;
    // the trial's G once, from walker 0's fresh bins (every bin is BT^stack_size), then broadcast
    for (int n = 0; n < nbins; ++n)
        AFQ_HIP(h, hipMemcpyAsync(h->th_stack + (long)n * per, h->th_BTpow, sizeof(double) * per, hipMemcpyDeviceToDevice, h->stream));
    AFQ_TRY(th_launch_greens<double>(h, h->th_stack, h->th_G0, nullptr, ts_first_bin(h, 0), 0, dim3(2)));
    AFQ_LAUNCH(h, thermal_reset_kernel, dim3((unsigned)((per + 255) / 256), h->nw), dim3(256), 0, h->stream, h->th_stack,
               h->th_G, h->weight, h->th_BTpow, h->th_G0, nbins, per, h->nw);
    AFQ_POST(h);
    h->th_slice = 0; h->th_block = 0; h->th_counter = 0;
    return AFQ_OK;
}

int afq_thermal_greens(afq_handle *h, int slice_ix) {
    AFQ_API(h, "afq_thermal_greens");
    if (!h) return AFQ_EINVAL;
    AFQ_TRY(th_need(h, false));
    if (slice_ix < 0 || slice_ix > h->th_L) AFQ_FAIL(h, AFQ_EINVAL, "afq_thermal_greens: slice_ix outside 0 .. ntime_slices");
    return th_complex(h) ? k_thermal_c_greens(h, slice_ix) : k_thermal_greens(h, slice_ix);
}

int afq_thermal_propagate(afq_handle *h, const double *u, int32_t *fields_out, double eshift) {
    AFQ_API(h, "afq_thermal_propagate");
    if (!h) return AFQ_EINVAL;
    AFQ_TRY(th_need(h, false));
    if (th_complex(h)) AFQ_FAIL(h, AFQ_ESTATE, "afq_thermal_propagate: continuous fields are configured (afq_thermal_propagate_continuous)");
    if (!u) AFQ_FAIL(h, AFQ_EINVAL, "afq_thermal_propagate: the uniforms f64[nw, M] are needed");
    if (h->th_slice >= h->th_L) AFQ_FAIL(h, AFQ_ESTATE, "afq_thermal_propagate: the path is complete (afq_thermal_reset starts the next)");
    const int M = h->M;
    AFQ_HIP(h, hipMemcpyAsync(h->th_u, u, sizeof(double) * (size_t)M * h->nw, hipMemcpyHostToDevice, h->stream));
    ThSliceArgs a;
    a.G = h->th_G; a.stack = h->th_stack; a.weight = h->weight; a.u = h->th_u; a.BH1 = h->th_BH1;
    a.fields = h->th_fields; a.M = M; a.nbins = h->th_nbins; a.block = h->th_block; a.counter = h->th_counter;
    for (int f = 0; f < 2; ++f) for (int s = 0; s < 2; ++s) { a.auxf[f][s] = h->th_auxf[f][s]; a.delta[f][s] = h->th_auxf[f][s] - 1.0; }
    a.exp_eshift = exp(eshift);
    if (th_delayed_slice(h))
        AFQ_TRY(th_launch<thermal_slice_delayed_kernel>(h, "thermal_slice_delayed_kernel", dim3(h->nw), th_slice_delayed_lds(M), a));
    else
        AFQ_TRY(th_launch<thermal_slice_kernel>(h, "thermal_slice_kernel", dim3(h->nw), th_slice_lds(M), a));
    th_advance(h);
    if (h->th_slice % h->th_nstblz == 0) AFQ_TRY(k_thermal_greens(h, h->th_slice - 1));
    if (h->th_slice < h->th_L)                          // (its LDS is beyond 64 KiB at M > 90)
        AFQ_TRY(th_launch<thermal_wrap_kernel>(h, "thermal_wrap_kernel", dim3(2 * h->nw), th_wrap_lds(M), h->th_G, h->th_BT, h->th_BTinv, M));
    if (fields_out) return copy_out(h, fields_out, h->th_fields, sizeof(int) * (size_t)M * h->nw);
    return AFQ_OK;
}

int afq_thermal_energy(afq_handle *h, double *E_out, double *nav_out) {
    AFQ_API(h, "afq_thermal_energy");
    if (!h) return AFQ_EINVAL;
    AFQ_TRY(th_need(h, false));
    if (!E_out && !nav_out) AFQ_FAIL(h, AFQ_EINVAL, "afq_thermal_energy: nothing asked for");
    if (th_complex(h)) return k_thermal_c_energy(h, E_out, nav_out);
    AFQ_TRY(ts_launch_rdm<double>(h, h->th_G, h->th_nav));
    AFQ_TRY(k_energy_hubbard_full_g(h, h->G, h->nw, h->energy));
    return th_energy_out(h, E_out, nav_out);
}

int afq_thermal_set_sweep_budget(afq_handle *h, size_t bytes) {
    if (!h) return AFQ_EINVAL;
    h->th_sw_budget = bytes;
    return AFQ_OK;
}

int afq_thermal_estimates(afq_handle *h, int what, double *cols_out, double *per_bin_out, double *one_rdm_out,
                          double *two_rdm_out) {
    AFQ_API(h, "afq_thermal_estimates");
    if (!h) return AFQ_EINVAL;
    AFQ_TRY(th_need(h, false));
    const bool avg = what & AFQ_THERMAL_EST_AVERAGE_GF, one = what & AFQ_THERMAL_EST_ONE_RDM, two = what & AFQ_THERMAL_EST_TWO_RDM;
    if (what & ~(AFQ_THERMAL_EST_AVERAGE_GF | AFQ_THERMAL_EST_ONE_RDM | AFQ_THERMAL_EST_TWO_RDM))
        AFQ_FAIL(h, AFQ_EINVAL, "afq_thermal_estimates: unknown bits in what");
    if (!cols_out || (one && !one_rdm_out) || (two && !two_rdm_out))
        AFQ_FAIL(h, AFQ_EINVAL, "afq_thermal_estimates: null output (cols_out always, one_rdm_out with ONE_RDM, two_rdm_out with TWO_RDM)");
    if (two && h->th_kind != TH_CPLX_DIAG)
        AFQ_FAIL(h, AFQ_EUNSUPPORTED, "afq_thermal_estimates: two_rdm is the structure factor of the UEG walkers (no Hubbard)");
    const bool cx = th_complex(h);
    if (avg && h->th_engine == TH_ENGINE_WIDE)
        AFQ_FAIL(h, AFQ_EUNSUPPORTED, cx ? "afq_thermal_estimates: average_gf is not supported on a wide_basis handle (AFQ_THERMAL_WIDE has no sweep kernel)"
                                         : "afq_thermal_estimates: average_gf is not supported on a delayed_updates handle (AFQ_THERMAL_DELAYED has no sweep kernel)");
    const int M = h->M, nw = h->nw, nbins = h->th_nbins, nbt = avg ? nbins : 1;
    const size_t mm = (size_t)M * M, n = nw, nq4 = two ? 4 * (size_t)h->nq : 0;
    // the small results, fetched in one copy: cols [nw, 4], per_bin [nbt, nw, 4], one_rdm [2, M, M], two_rdm c128 [2, 2, nq];
    // behind them the sweep's energies c128 [nbins, nw, 3] and nav [nbins, nw]
    const size_t o_cols = 0, o_bin = o_cols + sizeof(double) * 4 * n, o_rdm = o_bin + sizeof(double) * 4 * n * nbt,
                 o_two = th_up256(o_rdm + sizeof(double) * 2 * mm), o_end = o_two + sizeof(cplx) * nq4,
                 o_E = th_up256(o_end), o_nav = o_E + sizeof(cplx) * 3 * n * nbins, o_all = o_nav + sizeof(double) * n * nbins;
    AFQ_TRY(dev_grow(h, LT_WALKERS, &h->th_sw_out, &h->th_sw_out_len, o_all, "thermal estimates"));
    unsigned char *out = h->th_sw_out;
    double *cols = (double *)(out + o_cols), *per_bin = (double *)(out + o_bin), *rdm = (double *)(out + o_rdm);
    cplx *two_sum = (cplx *)(out + o_two), *two_src = nullptr;
    if (!avg) {
        // what update_thermal has always done: G at the handle's slice, then the energy's own launches
        AFQ_TRY(cx ? k_thermal_c_greens(h, h->th_slice) : k_thermal_greens(h, h->th_slice));
        AFQ_TRY(cx ? ts_launch_rdm<cplx>(h, h->thc_G, h->th_nav) : ts_launch_rdm<double>(h, h->th_G, h->th_nav));
        AFQ_TRY(th_energy_n(h, h->G, nw, h->energy, &two_src));
        AFQ_LAUNCH(h, thermal_sweep_reduce_kernel, dim3((nw + 127) / 128), dim3(128), 0, h->stream, h->energy, h->th_nav, nw, 1,
                   cols, per_bin);
        AFQ_POST(h);
    } else {
        // G [cb, nw, 2, M, M], P c128 of the same shape and the engine's own scratch for every work-group of the grid,
        // [cb, 2 nw, scratch(M)] (none for the resident engine): cb whole bins under the budget
        const size_t gsz = cx ? sizeof(cplx) : sizeof(double);
        const size_t b_P = sizeof(cplx) * 2 * mm * n, b_G = gsz * 2 * mm * n, b_T = gsz * 2 * n * th_greens_scratch(h);
        const size_t budget = h->th_sw_budget ? h->th_sw_budget : TH_SWEEP_BUDGET;
        size_t cb = budget / (b_P + b_G + b_T);
        cb = cb < 1 ? 1 : cb > (size_t)nbins ? (size_t)nbins : cb;
        AFQ_TRY(dev_grow(h, LT_WALKERS, &h->th_sw_ws, &h->th_sw_ws_len, cb * (b_P + b_G + b_T), "thermal estimates: the sweep's scratch"));
        cplx *P = (cplx *)h->th_sw_ws, *Ts = (cplx *)(h->th_sw_ws + cb * (b_P + b_G));
        void *Gs = h->th_sw_ws + cb * b_P;
        cplx *E = (cplx *)(out + o_E);
        double *nav = (double *)(out + o_nav);
        for (int ts0 = 0; ts0 < nbins; ts0 += (int)cb) {
            const int nb = nbins - ts0 < (int)cb ? nbins - ts0 : (int)cb;
            if (cx) {
                AFQ_TRY(k_thermal_c_sweep_greens(h, (cplx *)Gs, Ts, ts0, nb));
                AFQ_TRY(k_thermal_c_sweep_rdm(h, (const cplx *)Gs, P, nav + (size_t)ts0 * n, nb * nw));
            } else {
                AFQ_TRY(th_launch_greens<double>(h, h->th_stack, h->th_G, nullptr, 0, -1, dim3(2 * nw, nb), (double *)Gs, (double *)Ts, ts0));
                AFQ_TRY(ts_launch_rdm_n<double>(h, (const double *)Gs, P, nav + (size_t)ts0 * n, nb * nw));
            }
            AFQ_TRY(th_energy_n(h, P, nb * nw, E + 3 * (size_t)ts0 * n, &two_src));
            if (two_src) two_src += (size_t)(nb - 1) * n * nq4;       // (behind the loop: the path's last bin)
        }
        AFQ_LAUNCH(h, thermal_sweep_reduce_kernel, dim3((nw + 127) / 128), dim3(128), 0, h->stream, E, nav, nw, nbins, cols, per_bin);
        AFQ_POST(h);
    }
    if (one) {
        const long len = 2L * M * M;
        const dim3 grid((unsigned)((len + 127) / 128)), block(128);
        afq_note_launch(h, "thermal_one_rdm_kernel");
        if (cx) hipLaunchKernelGGL(thermal_one_rdm_kernel<cplx>, grid, block, 0, h->stream, h->thc_G, h->weight, nw, len, rdm);
        else hipLaunchKernelGGL(thermal_one_rdm_kernel<double>, grid, block, 0, h->stream, h->th_G, h->weight, nw, len, rdm);
        AFQ_POST(h);
    }
    if (two) AFQ_TRY(k_ueg_sf_wsum(h, two_src, nw, nullptr, h->weight, two_sum, nullptr));
    std::vector<unsigned char> host(o_end);
    AFQ_TRY(copy_out(h, host.data(), out, o_end));
    memcpy(cols_out, host.data() + o_cols, sizeof(double) * 4 * n);
    if (per_bin_out) memcpy(per_bin_out, host.data() + o_bin, sizeof(double) * 4 * n * nbt);
    if (one) memcpy(one_rdm_out, host.data() + o_rdm, sizeof(double) * 2 * mm);
    if (two) {
        const double *t = (const double *)(host.data() + o_two);
        for (size_t i = 0; i < nq4; ++i) two_rdm_out[i] = t[2 * i];
    }
    return AFQ_OK;
}

int afq_thermal_state(afq_handle *h, int32_t *out4) {
    if (!h || !out4) return AFQ_EINVAL;
    AFQ_TRY(th_need(h, false));
    out4[0] = h->th_slice; out4[1] = h->th_block; out4[2] = h->th_counter; out4[3] = h->th_nbins;
    return AFQ_OK;
}

}  // extern "C"
