// Per-walker small dense work: overlap matrices, LU (determinant + solve for
// the half-rotated Green's function), Gram-Schmidt re-orthogonalisation, the
// field shift / clipping, the phaseless weight update, population control and
// the mixed-estimator accumulation.  One workgroup per walker; panels live in
// LDS when they fit and in a global workspace otherwise.
#include <cstdlib>
#include <cstring>
#include <optional>
#include <type_traits>
#include "mfma_gemm.h"
#include "gj_wave.h"
#include "lds_dma.h"
#include "greens_small.h"

#include "block_scan.h"
#include "walker_fields.h"
#define NTHR 256

// --------------------------------------------------------------------------
__global__ void alive_kernel(const double *weight, int *alive, int nw) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w < nw) alive[w] = fabs(weight[w]) > 1e-8 ? 1 : 0;   // qmc/afqmc.py:232
}

int k_alive(afq_handle *h) {
    AFQ_LAUNCH(h, alive_kernel, dim3((h->nw + 255) / 256), dim3(256), 0, h->stream, h->weight,
                       h->alive, h->nw);
    AFQ_POST(h);
    return AFQ_OK;
}

// --------------------------------------------------------------------------
// LU with partial pivoting of an n x n complex matrix O (row-major, leading
// dimension n) held in LDS or global memory.  All NTHR threads cooperate.
// perm[i] = source row of pivoted row i.  Returns (on every thread) nothing;
// thread 0 accumulates phase and log|det| into *ph, *la.
__device__ inline void lu_factor(cplx *O, int n, int *perm, int *piv_s, cplx *ph, double *la) {
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += NTHR) perm[i] = i;
    if (tid == 0) { *ph = cmake(1.0, 0.0); *la = 0.0; }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
        // pivot search by wave 0: LAPACK izamax metric |re| + |im|
        if (tid < 64) {
            double best = -1.0; int bi = k;
            for (int i = k + tid; i < n; i += 64) {
                const cplx v = O[(long)i * n + k];
                const double m = fabs(v.x) + fabs(v.y);
                if (m > best) { best = m; bi = i; }
            }
            for (int off = 32; off > 0; off >>= 1) {
                const double ob = __shfl_down(best, off);
                const int oi = __shfl_down(bi, off);
                if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
            }
            if (tid == 0) *piv_s = bi;
        }
        __syncthreads();
        const int p = *piv_s;
        if (p != k) {
            for (int j = tid; j < n; j += NTHR) {
                const cplx t = O[(long)k * n + j];
                O[(long)k * n + j] = O[(long)p * n + j];
                O[(long)p * n + j] = t;
            }
            if (tid == 0) { const int t = perm[k]; perm[k] = perm[p]; perm[p] = t; }
        }
        __syncthreads();
        const cplx d = O[(long)k * n + k];
        if (tid == 0) {
            const double a = hypot(d.x, d.y);
            cplx u = cmake(d.x / a, d.y / a);
            if (p != k) u = cmake(-u.x, -u.y);
            *ph = cmul(*ph, u);
            *la += log(a);
        }
        for (int i = k + 1 + tid; i < n; i += NTHR) O[(long)i * n + k] = cdiv(O[(long)i * n + k], d);
        __syncthreads();
        const int m = n - k - 1;
        for (int e = tid; e < m * m; e += NTHR) {
            const int i = k + 1 + e / m, j = k + 1 + e % m;
            cplx v = O[(long)i * n + j];
            const cplx l = O[(long)i * n + k], u = O[(long)k * n + j];
            v.x = fma(-l.x, u.x, v.x); v.x = fma(l.y, u.y, v.x);
            v.y = fma(-l.x, u.y, v.y); v.y = fma(-l.y, u.x, v.y);
            O[(long)i * n + j] = v;
        }
        __syncthreads();
    }
}


// One workgroup per walker, spins in sequence.  O = phi_s^T conj(psi_s)
// (walkers/single_det.py:310,316); Ghalf_s = O^-1 phi_s^T solved column by
// column from the LU factors; det = prod over spins of det O.
__global__ __launch_bounds__(NTHR) void greens_kernel(GreensArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int perm[256];
    __shared__ int piv_s;
    __shared__ cplx ph_s;
    __shared__ double la_s;
    const int w = blockIdx.x, tid = threadIdx.x;
    if (a.only_alive && !a.alive[w]) return;
    const int M = a.M, nt = a.nt;
    const cplx *phi = a.phi + (long)w * M * nt;
    cplx phase = cmake(1.0, 0.0);
    double logabs = 0.0;
    for (int s = 0; s < 2; ++s) {
        const int n = s == 0 ? a.na : a.nb;
        const int off = s == 0 ? 0 : a.na;
        if (n == 0) continue;
        cplx *O = a.o_in_lds ? (cplx *)smem : a.ws + (long)w * ((a.na > a.nb ? a.na : a.nb) * (long)(a.na > a.nb ? a.na : a.nb));
        for (int e = tid; e < n * n; e += NTHR) {
            const int i = e / n, j = e % n;
            cplx acc = cmake(0.0, 0.0);
            for (int p = 0; p < M; ++p) {
                const cplx x = phi[(long)p * nt + off + i];
                const cplx y = a.psi[w * a.psi_stride + (long)p * nt + off + j];
                // x * conj(y)
                acc.x = fma(x.x, y.x, acc.x); acc.x = fma(x.y, y.y, acc.x);
                acc.y = fma(x.y, y.x, acc.y); acc.y = fma(-x.x, y.y, acc.y);
            }
            O[(long)i * n + j] = acc;
        }
        __syncthreads();
        lu_factor(O, n, perm, &piv_s, &ph_s, &la_s);
        if (tid == 0) { phase = cmul(phase, ph_s); logabs += la_s; }
        if (tid == 0 && s == 0 && a.det_a) { const double e0 = exp(logabs); a.det_a[w] = cmake(phase.x * e0, phase.y * e0); }
        if (a.ghalf) {
            // column c of Ghalf_s: solve L U x = P phi_s^T[:, c]
            cplx *gh = a.ghalf + ((long)w * nt + off) * M;
            for (int c = tid; c < M; c += NTHR) {
                for (int i = 0; i < n; ++i) {
                    cplx acc = phi[(long)c * nt + off + perm[i]];
                    for (int j = 0; j < i; ++j) {
                        const cplx l = O[(long)i * n + j], y = gh[(long)j * M + c];
                        acc.x = fma(-l.x, y.x, acc.x); acc.x = fma(l.y, y.y, acc.x);
                        acc.y = fma(-l.x, y.y, acc.y); acc.y = fma(-l.y, y.x, acc.y);
                    }
                    gh[(long)i * M + c] = acc;
                }
                for (int i = n - 1; i >= 0; --i) {
                    cplx acc = gh[(long)i * M + c];
                    for (int j = i + 1; j < n; ++j) {
                        const cplx u = O[(long)i * n + j], x = gh[(long)j * M + c];
                        acc.x = fma(-u.x, x.x, acc.x); acc.x = fma(u.y, x.y, acc.x);
                        acc.y = fma(-u.x, x.y, acc.y); acc.y = fma(-u.y, x.x, acc.y);
                    }
                    gh[(long)i * M + c] = cdiv(acc, O[(long)i * n + i]);
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double e = exp(logabs);
        a.det[w] = cmake(phase.x * e, phase.y * e);
    }
}


// --------------------------------------------------------------------------
static WeightArgs no_weight_args() {
    WeightArgs a;
    memset(&a, 0, sizeof(a));
    return a;
}

__global__ void weight_kernel(WeightArgs a) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= a.nw) return;
    weight_update_and_cap(a, w);
}

// --------------------------------------------------------------------------
// The fast Green's function kernel for N <= 45 electrons per spin: one work-group per walker around greens_small_body
// (greens_small.h, where the phases are described).
template <bool INVERSE, bool WGJ>
__global__ __launch_bounds__(512) void greens_small_kernel(GreensArgs a, WeightArgs wa) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int w = blockIdx.x;
    if (a.only_alive && !a.alive[w]) return;
    greens_small_body<INVERSE, WGJ>(a, wa, w, smem, false);
}

// --------------------------------------------------------------------------
// Green's function / overlap for AT MOST 8 ELECTRONS PER SPIN (round 5: the electron gas of BASELINE configs[1] has 7 + 7,
// the 4 x 4 Hubbard lattice 8 + 8).  greens_small_kernel spends three dependent phases of 4-5 us each on such a walker --
// two 16 x 16 MFMA tiles that are 80 % padding per phase and a 7-step register Gauss-Jordan built for n = 32 -- and the
// kernel is one work-group per CU in a single round, i.e. pure latency.  Here, on the vector ALU, with every lane busy:
//   phase 0  walker AND trial into LDS by LDS-DMA (one latency)
//   phase 1  O_s[i, j] = sum_p phi[p, i] conj(psi[p, j]): thread = (spin, i, j, quarter of the p range), quad reduction
//   phase 2  in-place Gauss-Jordan inverse with implicit row pivoting, one wave per spin, ONE LANE PER ELEMENT
//            (lane = 8 row + column): per pivot step the column and the pivot row reach every lane by two lane
//            permutes, the pivot row is found by the DPP maximum of gj_wave.h, and every lane does one complex FMA
//   phase 3  Ghalf_s[i, q] = sum_j O^-1[i, j] phi[q, j]: thread per output element, stores along q
// Same arguments, outputs and riders (weight update + cap behind the determinant, spin sum, per-walker trial of the
// back-propagation, O^-1 for the Hirsch propagator) as greens_small_kernel; walkers/single_det.py:295-321, :170-199.
template <bool INVERSE>
__global__ __launch_bounds__(512) void greens_tiny_kernel(GreensArgs a, WeightArgs wa) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ cplx O_l[2][64], oinv_l[2][64], piv_l[2][32];
    __shared__ int prow_l[2][32];
    __shared__ cplx ph_s[2];
    __shared__ int la_s[2];
    const int w = blockIdx.x, tid = threadIdx.x;
    if (a.only_alive && !a.alive[w]) return;
    const int M = a.M, nt = a.nt, na = a.na, nb = a.nb;
    cplx *phi_l = (cplx *)smem, *psi_l = phi_l + (long)M * nt;
    const int lane = tid & 63, wave8 = __builtin_amdgcn_readfirstlane(tid >> 6);
    {   // ---- phase 0
        const unsigned total = (unsigned)(M * nt) * 16u;
        const char *phi_g = (const char *)(a.phi + (long)w * M * nt), *psi_g = (const char *)(a.psi + w * a.psi_stride);
        for (unsigned b0 = (unsigned)wave8 * 1024u; b0 < total; b0 += 8 * 1024u) {
            const unsigned bo = b0 + (unsigned)lane * 16u;
            if (bo < total) { glds16(phi_g + bo, (char *)phi_l + b0); glds16(psi_g + bo, (char *)psi_l + b0); }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    {   // ---- phase 1: thread = (spin s, row i, column j, quarter c4 of the contraction)
        const int o = tid >> 2, c4 = tid & 3;
        const int s = o >> 6, i = (o >> 3) & 7, j = o & 7;
        const int ns = s ? nb : na, off = s ? na : 0;
        const bool live = i < ns && j < ns;
        const int ic = off + (live ? i : 0), jc = off + (live ? j : 0);
        double ar = 0.0, ai = 0.0;
        // (eight terms per trip: sixteen LDS reads in flight ahead of the FMAs instead of a read -> wait -> FMA chain per term)
        const int nterm = (M - c4 + 3) >> 2;
        for (int t0 = 0; t0 < nterm; t0 += 8) {
            cplx x[8], y[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int p_ = c4 + 4 * (t0 + u), pc = p_ < M ? p_ : c4;
                x[u] = phi_l[pc * nt + ic]; y[u] = psi_l[pc * nt + jc];
                if (p_ >= M) x[u] = cmake(0.0, 0.0);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {                          // x * conj(y)
                ar = fma(x[u].x, y[u].x, ar); ar = fma(x[u].y, y[u].y, ar);
                ai = fma(x[u].y, y[u].x, ai); ai = fma(-x[u].x, y[u].y, ai);
            }
        }
        ar += __shfl_xor(ar, 1); ai += __shfl_xor(ai, 1);
        ar += __shfl_xor(ar, 2); ai += __shfl_xor(ai, 2);
        // (rows and columns past the electron count: the identity, so that the padded matrix has the same determinant)
        if (c4 == 0) O_l[s][i * 8 + j] = live ? cmake(ar, ai) : cmake(i == j ? 1.0 : 0.0, 0.0);
        if (tid < 64) { piv_l[tid >> 5][tid & 31] = cmake(1.0, 0.0); prow_l[tid >> 5][tid & 31] = tid & 31; }
    }
    __syncthreads();
    // ---- phase 2: waves 0 and 1 (different SIMDs), spin = wave
    if (wave8 < 2) {
        const int s = wave8, n = s ? nb : na;
        const int r = lane >> 3, c = lane & 7;
        cplx v = O_l[s][lane];
        double wx = v.x, wy = v.y;
        bool used = r >= n;
        int mystep = r;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < n) {
                // column k to every lane of its row
                const int src = (lane & 0x38) | k;
                const double fx = __shfl(wx, src), fy = __shfl(wy, src);
                // pivot row: largest |re| + |im| among the rows not used yet (LAPACK's izamax metric on the top 26 bits of the
                // double, ties -> lowest row), as in gj_wave.h
                const unsigned mb = (unsigned)__double2hiint(fabs(fx) + fabs(fy));
                const unsigned key = used ? 0u : ((((mb >> 5) + 1u) << 5) | (unsigned)(31 - r));
                const int p_ = 31 - (int)(gj_wave_max_u32(key) & 31u);
                const bool isp = r == p_;
                // the pivot (uniform) and its reciprocal: v_rcp_f64 + two Newton steps
                const double dx = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(fx), p_ * 8),
                                                   __builtin_amdgcn_readlane(__double2loint(fx), p_ * 8));
                const double dy = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(fy), p_ * 8),
                                                   __builtin_amdgcn_readlane(__double2loint(fy), p_ * 8));
                // (every product-sum below is an explicit fma: the two instantiations of this kernel -- determinant only, and
                //  with the inverse -- must round alike, whatever the compiler would contract where)
                const double nn = fma(dx, dx, dy * dy);
                double dn = __builtin_amdgcn_rcp(nn);
                dn = fma(fma(-nn, dn, 1.0), dn, dn);
                dn = fma(fma(-nn, dn, 1.0), dn, dn);
                const double ix = dx * dn, iy = -dy * dn;
                // the pivot row, column k replaced by the unit entry, scaled by 1 / d
                const int psrc = p_ * 8 + c;
                double px = __shfl(wx, psrc), py = __shfl(wy, psrc);
                if (c == k) { px = 1.0; py = 0.0; }
                const double qx = fma(px, ix, -(py * iy)), qy = fma(px, iy, py * ix);
                if (isp) {
                    wx = qx; wy = qy; mystep = k;
                    if (c == 0) piv_l[s][k] = cmake(dx, dy);
                } else {
                    const double bx = c == k ? 0.0 : wx, by = c == k ? 0.0 : wy;
                    wx = fma(-fx, qx, bx); wx = fma(fy, qy, wx);
                    wy = fma(-fx, qy, by); wy = fma(-fy, qx, wy);
                }
                used = used || isp;
            }
        }
        if (c == 0 && r < n) prow_l[s][mystep] = r;
        __builtin_amdgcn_wave_barrier();
        // un-permuted inverse: A^-1[step(r)][prow[c]] = W[r][c]
        if (INVERSE && r < n && c < n) oinv_l[s][mystep * 8 + prow_l[s][c]] = cmake(wx, wy);
        cplx ph;
        int la;
        gj_wave_det(n, lane, piv_l[s], prow_l[s], ph, la);
        if (lane == 0) { ph_s[s] = ph; la_s[s] = la; }
    }
    __syncthreads();
    if (tid == 448) {
        const cplx p2 = cmul(ph_s[0], ph_s[1]);
        const int e = la_s[0] + la_s[1];
        a.det[w] = cmake(ldexp(p2.x, e), ldexp(p2.y, e));
        if (a.det_a) a.det_a[w] = cmake(ldexp(ph_s[0].x, la_s[0]), ldexp(ph_s[0].y, la_s[0]));
        if (wa.weight) weight_update_and_cap(wa, w);
    }
    if (!INVERSE) return;
    const int nmax = na > nb ? na : nb;
    if (a.oinv) {
        cplx *oo = a.oinv + (long)w * 2 * nmax * nmax;
        for (int e = tid; e < 2 * nmax * nmax; e += 512) {
            const int s = e / (nmax * nmax), rem = e - s * nmax * nmax, i = rem / nmax, j = rem - i * nmax;
            const int ns = s ? nb : na;
            if (i < ns && j < ns) oo[e] = oinv_l[s][i * 8 + j];
        }
    }
    if (!a.ghalf) return;
    // ---- phase 3
    auto ghalf_of = [&](const int s, const int i, const int q) {
        const int ns = s ? nb : na, off = s ? na : 0;
        double gr = 0.0, gi = 0.0;
        cplx x[8], y[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {                              // every read in flight before the first FMA
            const int jc = j < ns ? j : 0;
            x[j] = oinv_l[s][i * 8 + jc]; y[j] = phi_l[q * nt + off + jc];
            if (j >= ns) x[j] = cmake(0.0, 0.0);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            gr = fma(x[j].x, y[j].x, gr); gr = fma(-x[j].y, y[j].y, gr);
            gi = fma(x[j].x, y[j].y, gi); gi = fma(x[j].y, y[j].x, gi);
        }
        return cmake(gr, gi);
    };
    cplx *gh = a.ghalf + (long)w * nt * M;
    if (a.gsum) {                                              // na == nb (host-checked): both spins of an element in one thread
        cplx *gs = a.gsum + (long)w * na * M;
        for (int e = tid; e < na * M; e += 512) {
            const int i = e / M, q = e - i * M;
            const cplx ga = ghalf_of(0, i, q), gb = ghalf_of(1, i, q);
            if (!a.skip_spin) { gh[e] = ga; gh[(long)na * M + e] = gb; }
            gs[e] = cmake(ga.x + gb.x, ga.y + gb.y);
        }
    } else {
        for (int e = tid; e < nt * M; e += 512) {
            const int ii = e / M, q = e - ii * M;
            const int s = ii < na ? 0 : 1;
            gh[e] = ghalf_of(s, ii - (s ? na : 0), q);
        }
    }
}

// the one-work-group kernels: [with Ghalf or O^-1 | determinant only][tiny, wave Gauss-Jordan (N <= 32), blocked]; the
// dynamic-LDS cap of each is raised once per kernel and device, not per launch
typedef void (*GreensKernel)(GreensArgs, WeightArgs);
struct GreensVariant { GreensKernel kern; const char *name; size_t lds_set[AFQ_MAX_DEVICES]; };
#define GREENS_VARIANT(kern) {kern, #kern, {0}}
static GreensVariant greens_variants[2][3] = {
    {GREENS_VARIANT((greens_tiny_kernel<true>)), GREENS_VARIANT((greens_small_kernel<true, true>)),
     GREENS_VARIANT((greens_small_kernel<true, false>))},
    {GREENS_VARIANT((greens_tiny_kernel<false>)), GREENS_VARIANT((greens_small_kernel<false, true>)),
     GREENS_VARIANT((greens_small_kernel<false, false>))}};
#undef GREENS_VARIANT

// First half of an evaluation: the kernel's arguments and everything the evaluation means for the cached Green's function
// (version bump, closed-shell epoch, stamps, what the result says was skipped or rode along).  launch_greens launches what this
// has filled; the fused propagator runs gl.a / gl.wa as the tail of its own launch (k_prop_fused) behind the SAME bookkeeping.
static int greens_fill(afq_handle *h, cplx *ghalf, cplx *det, int only_alive, cplx *oinv, const GreensRequest &req,
                       GreensResult *res, GreensLaunch &gl) {
    GreensArgs &a = gl.a;
    a.oinv = oinv; a.gsum = nullptr;
    if (ghalf) h->gf.rewritten();
    a.M = h->M; a.na = h->na; a.nb = h->nb; a.nt = h->nt; a.nw = h->nw;
    a.phi = h->phi; a.psi = h->psi; a.psi_stride = h->psi_stride; a.ghalf = ghalf; a.det = det; a.ws = h->lu_ws;
    a.det_a = req.det_a;
    a.psi_real = h->psi_real && h->psi_stride == 0 && h->ndet <= 1;
    a.psi_closed = h->psi_closed && h->psi_stride == 0 && h->ndet <= 1;
    a.closed_bad = nullptr; a.closed_epoch = 0; a.counters = h->counters;
    if (ghalf == h->ghalf) h->gf.closed.clear();                // (set again below when THIS launch checks every walker)
    a.skip_spin = 0;
    const int nmax = h->na > h->nb ? h->na : h->nb;
    if (nmax > 256) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "more than 256 electrons per spin");
    // the step's weight update rides on the determinant kernel when the caller asked for it and this IS the overlap of the
    // propagated walkers
    gl.ride = req.ride_weight && res && det == h->ovlp_new && !only_alive && !oinv;
    gl.path = GreensLaunch::LU;
    if (k_greens_big_supported(h)) { gl.path = GreensLaunch::BIG; return AFQ_OK; }
    // (the fast kernel keeps the walker, both overlap matrices and their inverses in LDS: 160 KB per work-group)
    const size_t lds = sizeof(cplx) * (2 * ((size_t)nmax * nmax + 2 * nmax) + ((2 * nmax + 3) / 4 + 1) + (size_t)h->M * h->nt);
    if (nmax <= 45 && h->M <= 4 * GS_KSMAX && lds <= 160 * 1024) {
        gl.path = GreensLaunch::SMALL;
        a.o_in_lds = 1; a.only_alive = only_alive; a.alive = h->alive;
        gl.wa = gl.ride ? k_weight_args(h, req.eshift) : no_weight_args();
        if (gl.ride) res->weight_rode = true;
        gl.wgj = nmax <= 32;
        // at most 8 electrons per spin, walker + trial in LDS: the vector-ALU kernel above
        const size_t lds_tiny = sizeof(cplx) * 2 * (size_t)h->M * h->nt;
        gl.tiny = nmax <= 8 && h->nt >= 1 && lds_tiny <= 150 * 1024;
        gl.inverse = ghalf || oinv;
        // the spin sum the force bias contracts (every walker written: not on the only_alive path)
        const bool want_sum = ghalf && ghalf == h->ghalf && !only_alive && k_fb_use_sum(h) && h->psi_stride == 0;
        if (want_sum) {
            AFQ_TRY(dev_ensure(h, LT_WALKERS, &h->ghalf_sum, (size_t)h->na * h->M * h->nw));
            a.gsum = h->ghalf_sum;
            if (req.may_skip_store && (gl.wgj || gl.tiny) && !oinv) { a.skip_spin = 1; if (res) res->store_skipped = true; }
        }
        if (want_sum && gl.wgj && !gl.tiny && a.psi_closed && !oinv) {
            // this launch compares the spin blocks of EVERY walker: its verdict holds for the Ghalf it leaves behind
            a.closed_bad = h->closed_bad; a.closed_epoch = ++h->closed_epoch;
            h->gf.closed.mark(h->gf);
        }
        gl.lds = gl.tiny ? lds_tiny : lds;
        if (want_sum) h->gf.gsum.mark(h->gf);
    }
    return AFQ_OK;
}

static int launch_greens(afq_handle *h, cplx *ghalf, cplx *det, int only_alive, cplx *oinv = nullptr,
                         const GreensRequest &req = GreensRequest(), GreensResult *res = nullptr) {
    GreensLaunch gl;
    AFQ_TRY(greens_fill(h, ghalf, det, only_alive, oinv, req, res, gl));
    GreensArgs &a = gl.a;
    if (gl.path == GreensLaunch::BIG) {
        GreensRequest big = req;
        big.ride_weight = gl.ride && h->ndet <= 1;
        return k_greens_big(h, ghalf, det, oinv, big, res);
    }
    if (gl.path == GreensLaunch::SMALL) {
        GreensVariant &v = greens_variants[gl.inverse ? 0 : 1][gl.tiny ? 0 : gl.wgj ? 1 : 2];
        {
            std::optional<KernelTrace> kt;
            if (gl.inverse) kt.emplace(h, AFQ_K_GREENS);
            AFQ_HIP(h, afq_raise_lds((const void *)v.kern, gl.lds, v.lds_set));
            afq_note_launch(h, v.name);
            hipLaunchKernelGGL(v.kern, dim3(h->nw), dim3(512), gl.lds, h->stream, a, gl.wa);
        }
        AFQ_POST(h);
        return AFQ_OK;
    }
    const int nmax = h->na > h->nb ? h->na : h->nb;
    if (oinv) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "inverse overlaps: the walker and both overlap matrices must fit 160 KB of LDS (N <= 45) or N > 45");
    const size_t need = sizeof(cplx) * (size_t)nmax * nmax;
    a.o_in_lds = need <= 64 * 1024;
    a.only_alive = only_alive; a.alive = h->alive;
    if (!a.o_in_lds && !h->lu_ws)
        AFQ_TRY(dev_alloc(h, LT_WALKERS, &h->lu_ws, (size_t)h->nw * nmax * nmax));
    a.ws = h->lu_ws;
    AFQ_LAUNCH(h, greens_kernel, dim3(h->nw), dim3(NTHR), a.o_in_lds ? need : 0, h->stream, a);
    AFQ_POST(h);
    return AFQ_OK;
}

// The end-of-step evaluation (Ghalf of the propagated walkers, their overlaps into ovlp_new) filled here and run by the fused
// propagator as the tail of its launch; the caller (afq_api.hip) has checked that the step is one the tail serves, and this
// confirms what the fill granted: the kernel the tail is (greens_small_body<true, true>) and the spin sum the next force bias
// contracts.  The per-spin store and the weight update ride or not, as requested (run-time fields of the arguments).
int k_prop_fused_greens(afq_handle *h, const GreensRequest &req, GreensResult *res, bool mul3) {
    GreensLaunch gl;
    AFQ_TRY(greens_fill(h, h->ghalf, h->ovlp_new, 0, nullptr, req, res, gl));
    if (gl.path != GreensLaunch::SMALL || !gl.wgj || gl.tiny || !gl.inverse || !gl.a.gsum || res->weight_rode != req.ride_weight)
        AFQ_FAIL(h, AFQ_ESTATE, "internal: the fused step's Green's function is not the one the propagator's tail evaluates");
    return k_prop_fused(h, &gl, mul3);
}

int k_greens(afq_handle *h, cplx *det_out, const GreensRequest &req, GreensResult *res) {
    return launch_greens(h, h->ghalf, det_out, 0, nullptr, req, res);
}
// det(psi^H phi) == det(phi^T conj(psi)) (transpose), so the same factorisation serves
// walkers/single_det.py:170-199
int k_overlap(afq_handle *h, cplx *det_out, const GreensRequest &req, GreensResult *res) {
    return launch_greens(h, nullptr, det_out, 0, nullptr, req, res);
}
// O^-1 of every walker and spin (+ determinant), no Ghalf: the discrete Hirsch propagator's inverse overlap
int k_inverse_overlap(afq_handle *h, cplx *oinv, cplx *det_out) {
    const int nmax = h->na > h->nb ? h->na : h->nb;
    if (!k_greens_big_supported(h) && (nmax > 45 || h->M > 4 * GS_KSMAX))
        AFQ_FAIL(h, AFQ_EUNSUPPORTED, "inverse overlaps: N <= 128 per spin (N <= 45: M <= 128)");
    return launch_greens(h, nullptr, det_out, 1, oinv);
}

// --------------------------------------------------------------------------
// force bias from the contraction output, per system
struct XbarArgs {
    int kind, flags, M, K, na, nb, nt, nw, nsplit, nq;
    double sqrt_dt, U;
    const cplx *vbias, *mf, *ghalf, *psi;
    const cplx *psicT;      // conj(psi)^T [nt, M] or null
    const cplx *gdiag;      // Hubbard: diag(G_s) partial sums [2 nw, gparts, M] left by the Ghalf GEMM, or null
    int gparts;
    cplx *xbar;
    int ndet;               // > 1: vbias holds ndet slices of det_stride elements, combined with detw
    long det_stride;
    const cplx *detw;       // [nw, ndet]
    // Hubbard with continuous fields: the kernel that makes the shifted fields also makes the HS potential's diagonal and
    // its degree-n Taylor factor per site (vhs_hubbard_kernel + exp_diag_factor_kernel of k_models.hip: two launches of
    // M nw elements each), hub_fac [nw, nv, M]; null otherwise
    cplx *hub_fac = nullptr;
    double hub_f = 0.0;     // sqrt(dt) sqrt(U) (charge decomposition: d = i f x) or sqrt(dt U) (spin: d = -+ f x)
    int hub_spin = 0, hub_order = 0;
};

__device__ inline cplx xbar_value(const XbarArgs &a, int w, int n) {
    cplx out = cmake(0.0, 0.0);
    if (a.flags & AFQ_PROP_FORCE_BIAS) {
        if (a.kind == AFQ_SYS_GENERIC) {
            // propagation/generic.py:150-152: -sqrt(dt) (i vbias - mf_shift)
            cplx v = cmake(0.0, 0.0);
            if (a.ndet > 1) {
                // propagation/generic.py:154-157 + walkers/multi_det.py:283-290:
                // vbias_n = sum_d w_d <V_n G_d> / sum_d w_d; <V_n G_d> = rchol_d^T vec(Ghalf_d)
                cplx num = cmake(0.0, 0.0), den = cmake(0.0, 0.0);
                for (int d = 0; d < a.ndet; ++d) {
                    const cplx wd = a.detw[(long)w * a.ndet + d];
                    if (wd.x == 0.0 && wd.y == 0.0) continue;     // skipped determinant (msd_combine_kernel): its Ghalf may hold anything
                    cplx x = cmake(0.0, 0.0);
                    const cplx *vb = a.vbias + (long)d * a.det_stride;
                    for (int b = 0; b < 2 * a.nsplit; ++b) x = cadd(x, vb[((long)b * a.nw + w) * a.K + n]);
                    cfma(num, wd, x);
                    den = cadd(den, wd);
                }
                v = cdiv(num, den);
            } else {
                // fixed summation order, four partial slices in flight at a time
                const int nb2 = 2 * a.nsplit;
                const cplx *vb = a.vbias + (long)w * a.K + n;
                const long bs = (long)a.nw * a.K;
                int b = 0;
                for (; b + 3 < nb2; b += 4) {
                    const cplx t0 = vb[b * bs], t1 = vb[(b + 1) * bs], t2 = vb[(b + 2) * bs], t3 = vb[(b + 3) * bs];
                    v = cadd(cadd(cadd(cadd(v, t0), t1), t2), t3);
                }
                for (; b < nb2; ++b) v = cadd(v, vb[b * bs]);
            }
            const cplx m = a.mf[n];
            out = cmake(-a.sqrt_dt * (-v.y - m.x), -a.sqrt_dt * (v.x - m.y));
        } else if (a.kind == AFQ_SYS_HUBBARD) {
            // diag of G_s = conj(psi_s) Ghalf_s at site n
            cplx g[2] = {cmake(0.0, 0.0), cmake(0.0, 0.0)};
            if (a.gdiag) {
                for (int s = 0; s < 2; ++s)
                    for (int pt = 0; pt < a.gparts; ++pt) g[s] = cadd(g[s], a.gdiag[((long)(2 * w + s) * a.gparts + pt) * a.M + n]);
            } else
            for (int s = 0; s < 2; ++s) {
                const int ns = s == 0 ? a.na : a.nb, off = s == 0 ? 0 : a.na;
                for (int i = 0; i < ns; ++i) {
                    // adjacent threads = adjacent sites n: both operands read along n
                    const cplx c = a.psicT ? a.psicT[(long)(off + i) * a.M + n] : cconj(a.psi[(long)n * a.nt + off + i]);
                    cfma(g[s], c, a.ghalf[((long)w * a.nt + off + i) * a.M + n]);
                }
            }
            const cplx m = a.mf[n];
            const double su = sqrt(a.U);
            cplx vb;
            if (a.flags & AFQ_PROP_HUBBARD_SPIN) {       // propagation/hubbard.py:472
                vb = cmake(su * (g[0].x - g[1].x), su * (g[0].y - g[1].y));
            } else {                                      // propagation/hubbard.py:406: i sqrt(U) (n_up + n_dn)
                const cplx t = cadd(g[0], g[1]);
                vb = cmake(-su * t.y, su * t.x);
            }
            out = cmake(-a.sqrt_dt * (vb.x - m.x), -a.sqrt_dt * (vb.y - m.y));
        } else {
            // UEG: propagation/planewave.py:76 (vbias filled by the sparse kernel)
            const cplx v = a.vbias[(long)w * a.K + n];
            out = cmake(-a.sqrt_dt * v.x, -a.sqrt_dt * v.y);
        }
    }
    return out;
}

__global__ void xbar_kernel(XbarArgs a) {
    const int w = blockIdx.y;
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= a.K) return;
    a.xbar[(long)w * a.K + n] = xbar_value(a, w, n);
}

static XbarArgs xbar_args(afq_handle *h) {
    XbarArgs a;
    a.kind = h->kind; a.flags = h->flags; a.M = h->M; a.K = h->K; a.na = h->na; a.nb = h->nb;
    a.nt = h->nt; a.nw = h->nw; a.nsplit = h->fb_split; a.nq = h->nq;
    a.sqrt_dt = h->sqrt_dt; a.U = h->U;
    a.vbias = h->vbias; a.mf = h->mf_shift; a.ghalf = h->ghalf; a.psi = h->psi; a.xbar = h->xbar;
    a.psicT = (h->ndet <= 1 && h->psi_stride == 0) ? h->psicT : nullptr;
    a.gdiag = (h->kind == AFQ_SYS_HUBBARD && h->gdiag && h->gf.gdiag.current(h->gf)) ? h->gdiag : nullptr;
    a.gparts = h->gdiag_parts;
    a.ndet = h->ndet; a.detw = h->detw; a.det_stride = (long)2 * h->fb_split * h->nw * h->K;
    if (h->ndet > 1) a.vbias = h->vbias_all;
    // (the contraction with the determinant-averaged G left ONE set of partials, already weighted: k_force_bias_msd_gbar)
    if (h->ndet > 1 && h->msd_fb_gbar && h->kind == AFQ_SYS_GENERIC) a.ndet = 1;
    return a;
}

int k_xbar(afq_handle *h) {
    const XbarArgs a = xbar_args(h);
    AFQ_LAUNCH(h, xbar_kernel, dim3((h->K + 127) / 128, h->nw), dim3(128), 0, h->stream, a);
    AFQ_POST(h);
    return AFQ_OK;
}

// --------------------------------------------------------------------------
// multi-determinant trial: weights and weighted averages (walkers/multi_det.py:194-229,135-162)
// skip_small (Green's function, walkers/multi_det.py:209,218): a determinant whose overlap with the walker is below 1e-16 is
// left out -- the reference `continue`s past it, keeping whatever Gi / weight the walker object held before (zeros for a fresh
// walker); here it gets the weight 0 and every consumer of the weights (force bias, energy) passes over it, i.e. the
// reference's result for a fresh walker.  A singular overlap matrix may leave NaN as its determinant (0 x inf behind a zero
// pivot): that IS a zero overlap, in the Green's function and in calc_overlap (multi_det.py:135-162, which skips nothing);
// every such event is counted (afq_counters_ext [6]) so that a NaN from a genuine numerical failure does not pass unseen.
// The reference tests the alpha determinant first (:209) and the product of both second (:218): both tests are applied, the
// first on detd_a (the alpha determinant alone, written by the Green's function kernels beside the product).
__global__ void msd_combine_kernel(const cplx *detd, const cplx *detd_a, const cplx *coeffs, cplx *detw, cplx *det_out, int nw,
                                   int ndet, int skip_small, unsigned long long *counters) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    cplx tot = cmake(0.0, 0.0);
    for (int d = 0; d < ndet; ++d) {
        cplx dd = detd[(long)d * nw + w];
        const double mag = hypot(dd.x, dd.y);
        bool skip = skip_small && mag < 1e-16;
        if (skip_small && detd_a) {
            const cplx da = detd_a[(long)d * nw + w];
            const double ma = hypot(da.x, da.y);
            skip = skip || ma < 1e-16;
        }
        if (!(mag == mag)) { skip = true; if (counters) atomicAdd(&counters[6], 1ull); }
        if (skip) dd = cmake(0.0, 0.0);
        const cplx wd = cmul(cconj(coeffs[d]), dd);
        detw[(long)w * ndet + d] = wd;
        tot = cadd(tot, wd);
    }
    det_out[w] = tot;
}

int k_msd_combine(afq_handle *h, cplx *det_out, bool skip_small) {
    AFQ_LAUNCH(h, msd_combine_kernel, dim3((h->nw + 127) / 128), dim3(128), 0, h->stream, h->detd,
                       skip_small ? h->detd_a : nullptr, h->coeffs, h->detw, det_out, h->nw, h->ndet, skip_small ? 1 : 0, h->counters);
    AFQ_POST(h);
    return AFQ_OK;
}

// estimators/mixed.py:439-448: E = sum_d w_d E[G_d] / sum_d w_d, component-wise
__global__ void msd_energy_combine_kernel(const cplx *energy_all, const cplx *detw, cplx *energy, int nw,
                                          int ndet) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    cplx num[3] = {cmake(0.0, 0.0), cmake(0.0, 0.0), cmake(0.0, 0.0)}, den = cmake(0.0, 0.0);
    for (int d = 0; d < ndet; ++d) {
        const cplx wd = detw[(long)w * ndet + d];
        if (wd.x == 0.0 && wd.y == 0.0) continue;              // skipped determinant: its energy may be anything
        for (int c = 0; c < 3; ++c) cfma(num[c], wd, energy_all[((long)d * nw + w) * 3 + c]);
        den = cadd(den, wd);
    }
    for (int c = 0; c < 3; ++c) energy[(long)w * 3 + c] = cdiv(num[c], den);
}

int k_msd_energy_combine(afq_handle *h) {
    AFQ_LAUNCH(h, msd_energy_combine_kernel, dim3((h->nw + 127) / 128), dim3(128), 0, h->stream,
                       h->energy_all, h->detw, h->energy, h->nw, h->ndet);
    AFQ_POST(h);
    return AFQ_OK;
}

#include "philox.h"

// --------------------------------------------------------------------------
__device__ inline double block_sum(double v, double *red) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
    return t;
}

// propagation/continuous.py:140-158: clip, shift, constant factors
// FUSED: the force bias of (w, n) is evaluated here from the contraction output (xbar_value) instead
// of being read back from a separate xbar_kernel launch
// rng.on: the auxiliary fields are drawn here from the device stream instead of being read from xi (the same
// numbers rng_normal_kernel writes: element e = w K + n is member e & 1 of Philox pair e >> 1), and the alive
// flag of the step (qmc/afqmc.py:232) is set here too -- one launch less per step.

template <bool FUSED>
__global__ __launch_bounds__(NTHR) void fields_kernel(int K, double sqrt_dt, const double *xi, cplx *xbar,
                                                      const cplx *mf, cplx *xs, cplx *cmf, cplx *cfb,
                                                      unsigned long long *counters, const int *alive, XbarArgs xa,
                                                      FieldRng rng) {
    __shared__ double red[NTHR / 64][8];
    const int w = blockIdx.x;
    if (rng.on) {
        const bool live = fabs(rng.weight[w]) > 1e-8;
        if (threadIdx.x == 0) rng.alive_out[w] = live ? 1 : 0;
        if (!live) return;
    } else if (alive && !alive[w]) return;
    // sums: mean-field shift (re, im), xi . xbar (re, im), xbar . xbar (re, im), clipped count
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};
    // (the force bias and the mean-field shift of a field are REQUESTED before its Philox arithmetic and used behind it:
    //  the kernel is one short latency chain per work-group, and the loads now fly under the ~1 us of integer / log / sincos)
    auto element = [&](const long e, const int n, const double xdev, cplx b, const cplx mm) {
        const double ab = hypot(b.x, b.y);
        if (ab > 1.0) { b.x /= ab; b.y /= ab; acc[6] += 1.0; }
        const double x = rng.on ? xdev : xi[e];
        const cplx sft = cmake(x - b.x, -b.y);
        {
        xbar[e] = b;
        xs[e] = sft;
        }
        if (FUSED && xa.hub_fac) {
            // propagation/hubbard.py:409-413 / :475-480, continuous.py:104-107 with a diagonal potential: one factor per site
            auto taylor = [&](const cplx d) {
                cplx acc = cmake(1.0, 0.0), t = acc;
                for (int k = 1; k <= xa.hub_order; ++k) {
                    t = cmul(d, t);
                    t = cmake(t.x / k, t.y / k);
                    acc = cadd(acc, t);
                }
                return acc;
            };
            if (!xa.hub_spin) xa.hub_fac[(long)w * K + n] = taylor(cmake(-xa.hub_f * sft.y, xa.hub_f * sft.x));
            else {
                xa.hub_fac[((long)w * 2 + 0) * K + n] = taylor(cmake(-xa.hub_f * sft.x, -xa.hub_f * sft.y));
                xa.hub_fac[((long)w * 2 + 1) * K + n] = taylor(cmake(xa.hub_f * sft.x, xa.hub_f * sft.y));
            }
        }
        acc[0] += sft.x * mm.x - sft.y * mm.y;
        acc[1] += sft.x * mm.y + sft.y * mm.x;
        acc[2] += x * b.x; acc[3] += x * b.y;
        acc[4] += b.x * b.x - b.y * b.y;
        acc[5] += 2.0 * b.x * b.y;
    };
    const long e0 = (long)w * K;
    if (K <= NTHR) {
        // a thread per field (a Philox pair is then generated by both of its threads): with few fields the evaluation of the
        // force bias (xbar_value: a contraction per element for the lattice models) wants every thread of the work-group
        const int n = threadIdx.x;
        if (n < K) {
            const cplx b = FUSED ? xbar_value(xa, w, n) : xbar[e0 + n];
            const cplx mm = mf[n];
            double xn[2] = {0.0, 0.0};
            if (rng.on) philox_normal_pair((e0 + n) >> 1, rng.seed, rng.stream, rng.counter, xn[0], xn[1]);
            element(e0 + n, n, xn[(e0 + n) & 1], b, mm);
        }
    } else {
        // a thread takes the two members of one Philox pair (elements 2 p, 2 p + 1 of the stream: consecutive fields of
        // this walker, or its first / last field alone when the walker's K fields start or end inside a pair), so that a
        // pair is generated once -- with a thread per field every pair was generated twice and one normal of each thrown away
        // Generic Hamiltonian, one determinant, force bias on (the C3 step): the 2 x 2 nsplit split-K partial sums of the pair's
        // two fields and their mean-field shifts are loaded in ONE flight, no branch between them -- the partials come from the
        // other XCDs' force-bias work-groups (16 MB at C3), and this kernel is their round trips: 5.3 of its 10.7 us with the
        // loads of one field at a time, four in flight (round 6; the sums keep xbar_value's order: bit-identical)
        const bool flight = FUSED && xa.kind == AFQ_SYS_GENERIC && xa.ndet <= 1 && (xa.flags & AFQ_PROP_FORCE_BIAS) && !xa.hub_fac;
        for (long pr = (e0 >> 1) + threadIdx.x; pr <= ((e0 + K - 1) >> 1); pr += NTHR) {
            cplx bb[2] = {cmake(0.0, 0.0), cmake(0.0, 0.0)}, mm[2] = {cmake(0.0, 0.0), cmake(0.0, 0.0)};
            if (flight) {
                int nn[2];
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const int n = (int)(2 * pr + m - e0);
                    nn[m] = n < 0 ? 0 : n >= K ? K - 1 : n;          // (a pair that straddles the walker: a valid address, value unused)
                }
                const int nb2 = 2 * xa.nsplit;
                const long bs = (long)xa.nw * K;
                const cplx *vb0 = xa.vbias + (long)w * K + nn[0], *vb1 = xa.vbias + (long)w * K + nn[1];
                mm[0] = mf[nn[0]]; mm[1] = mf[nn[1]];
                cplx v0 = cmake(0.0, 0.0), v1 = cmake(0.0, 0.0);
                int b = 0;
                for (; b + 7 < nb2; b += 8) {
                    cplx t0[8], t1[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) { t0[j] = vb0[(b + j) * bs]; t1[j] = vb1[(b + j) * bs]; }
#pragma unroll
                    for (int j = 0; j < 8; ++j) { v0 = cadd(v0, t0[j]); v1 = cadd(v1, t1[j]); }
                }
                for (; b + 3 < nb2; b += 4) {
                    cplx t0[4], t1[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) { t0[j] = vb0[(b + j) * bs]; t1[j] = vb1[(b + j) * bs]; }
#pragma unroll
                    for (int j = 0; j < 4; ++j) { v0 = cadd(v0, t0[j]); v1 = cadd(v1, t1[j]); }
                }
                for (; b < nb2; ++b) { v0 = cadd(v0, vb0[b * bs]); v1 = cadd(v1, vb1[b * bs]); }
                // propagation/generic.py:150-152 (xbar_value): -sqrt(dt) (i vbias - mf_shift)
                bb[0] = cmake(-xa.sqrt_dt * (-v0.y - mm[0].x), -xa.sqrt_dt * (v0.x - mm[0].y));
                bb[1] = cmake(-xa.sqrt_dt * (-v1.y - mm[1].x), -xa.sqrt_dt * (v1.x - mm[1].y));
            } else
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const long e = 2 * pr + m;
                const int n = (int)(e - e0);
                if (n >= 0 && n < K) { bb[m] = FUSED ? xbar_value(xa, w, n) : xbar[e]; mm[m] = mf[n]; }
            }
            double xn[2] = {0.0, 0.0};
            if (rng.on) philox_normal_pair(pr, rng.seed, rng.stream, rng.counter, xn[0], xn[1]);
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const long e = 2 * pr + m;
                const int n = (int)(e - e0);
                if (n >= 0 && n < K) element(e, n, xn[m], bb[m], mm[m]);
            }
        }
    }
    // one reduction for all seven sums: wave shuffles, one barrier
#pragma unroll
    for (int q = 0; q < 7; ++q)
        for (int off = 32; off > 0; off >>= 1) acc[q] += __shfl_down(acc[q], off);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 7; ++q) red[threadIdx.x >> 6][q] = acc[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            t[q] = 0.0;
            for (int i = 0; i < NTHR / 64; ++i) t[q] += red[i][q];
        }
        cmf[w] = cmake(-sqrt_dt * t[0], -sqrt_dt * t[1]);
        cfb[w] = cmake(t[2] - 0.5 * t[4], t[3] - 0.5 * t[5]);
        if (t[6] > 0 && counters) atomicAdd(&counters[0], (unsigned long long)t[6]);
    }
}

int k_fields(afq_handle *h) {
    AFQ_LAUNCH(h, fields_kernel<false>, dim3(h->nw), dim3(NTHR), 0, h->stream, h->K, h->sqrt_dt, h->xi, h->xbar,
                       h->mf_shift, h->xs, h->cmf, h->cfb, h->counters, h->alive, XbarArgs(), FieldRng());
    AFQ_POST(h);
    return AFQ_OK;
}

// force bias from the contraction output + clip + shift in one launch (the step's hot path)
int k_xbar_fields(afq_handle *h, cplx *hubbard_factors) {
    FieldRng rng = FieldRng();
    if (h->rng_inline) {
        rng.on = 1; rng.seed = h->rng_seed; rng.stream = h->rng_stream; rng.counter = h->rng_inline_counter;
        rng.weight = h->weight; rng.alive_out = h->alive;
        h->rng_inline = false;
    }
    XbarArgs xa = xbar_args(h);
    if (hubbard_factors) {
        const bool spin = (h->flags & AFQ_PROP_HUBBARD_SPIN) != 0;
        xa.hub_fac = hubbard_factors; xa.hub_spin = spin ? 1 : 0; xa.hub_order = h->exp_order;
        xa.hub_f = spin ? sqrt(h->dt * h->U) : h->sqrt_dt * sqrt(h->U);
    }
    AFQ_LAUNCH(h, fields_kernel<true>, dim3(h->nw), dim3(NTHR), 0, h->stream, h->K, h->sqrt_dt, h->xi, h->xbar,
                       h->mf_shift, h->xs, h->cmf, h->cfb, h->counters, h->alive, xa, rng);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_fields_explicit(afq_handle *h, const double *xi_d, const cplx *xbar_d, cplx *xs_d, cplx *cmf_d,
                      cplx *cfb_d) {
    AFQ_LAUNCH(h, fields_kernel<false>, dim3(h->nw), dim3(NTHR), 0, h->stream, h->K, h->sqrt_dt, xi_d,
                       (cplx *)xbar_d, h->mf_shift, xs_d, cmf_d, cfb_d, (unsigned long long *)nullptr,
                       (const int *)nullptr, XbarArgs(), FieldRng());
    AFQ_POST(h);
    return AFQ_OK;
}

// FieldConfig.update: append this step's shifted fields to the walker's history
__global__ void bp_push_kernel(const cplx *xs, cplx *hist, int *bp_n, const int *flag, int K, int nbp) {
    const int w = blockIdx.x;
    if (!flag[w]) return;
    const int n = bp_n[w];
    if (n < nbp)
        for (int k = threadIdx.x; k < K; k += blockDim.x) hist[((long)w * nbp + n) * K + k] = xs[(long)w * K + k];
    __syncthreads();
    if (threadIdx.x == 0 && n < nbp) bp_n[w] = n + 1;
}

// fields of back-propagation step i (most recent first): B(x)^H = B(-conj(x)) for real symmetric L_n
__global__ void bp_fields_kernel(const cplx *hist, const int *bp_n, cplx *xs, int *alive, int K, int nbp, int i) {
    const int w = blockIdx.x;
    const int n = bp_n[w];
    const bool on = i < n;
    if (threadIdx.x == 0) alive[w] = on ? 1 : 0;
    if (!on) return;
    const cplx *src = hist + ((long)w * nbp + (n - 1 - i)) * K;
    for (int k = threadIdx.x; k < K; k += blockDim.x) xs[(long)w * K + k] = cmake(-src[k].x, src[k].y);
}

__global__ void bp_init_kernel(const cplx *phi0, cplx *phi_bp, long per, int nw) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i < per * nw) phi_bp[i] = phi0[i % per];
}

__global__ void conj_copy_kernel(const cplx *src, cplx *dst, long n) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i < n) dst[i] = cconj(src[i]);
}

__global__ void conj_transpose_kernel(const cplx *A, cplx *At, int M) {      // per spin: At = A^H
    const int s = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * M) return;
    const int r = i / M, c = i % M;
    At[(long)s * M * M + c * M + r] = cconj(A[(long)s * M * M + i]);
}

// estimators/back_propagation.py:187-207: est[3] += w, est[4:] += w G_bp, w = weight (x restored factor)
__global__ void bp_accumulate_kernel(const cplx *G, const double *weight, const double *bp_cos, const cplx *bp_ph,
                                     cplx *est, int nw, long gsz, int restore, const cplx *energy) {
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (e > gsz + 3) return;
    if (e > gsz && !energy) return;
    cplx acc = cmake(0.0, 0.0);
    for (int w = 0; w < nw; ++w) {
        cplx wt = cmake(weight[w], 0.0);
        if (restore == 1) wt = cmul(wt, bp_ph[w]);                                       // BP-PRes (partial)
        else if (restore == 2) wt = cmul(wt, cmake(bp_ph[w].x / bp_cos[w], bp_ph[w].y / bp_cos[w]));   // full
        if (e == gsz) acc = cadd(acc, wt);
        else if (e > gsz) cfma(acc, wt, energy[3 * w + (e - gsz - 1)]);      // estimates[:nreg] += weight * energies
        else cfma(acc, wt, G[(long)w * gsz + e]);
    }
    if (e == gsz) est[3] = cadd(est[3], acc);
    else if (e > gsz) est[e - gsz - 1] = cadd(est[e - gsz - 1], acc);
    else est[4 + e] = cadd(est[4 + e], acc);
}

// keep_mod > 0 (discrete fields, bp_n counts single fields): FieldConfig.reset zeroes `step` but not the position
// `ib` inside an unfinished configuration (walkers/stack.py:124-127)
__global__ void bp_reset_kernel(int *bp_n, double *bp_cos, cplx *bp_ph, int nw, int keep_mod) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w < nw) { bp_n[w] = keep_mod > 0 ? bp_n[w] % keep_mod : 0; bp_cos[w] = 1.0; bp_ph[w] = cmake(1.0, 0.0); }
}

int k_bp_push(afq_handle *h) {
    AFQ_LAUNCH(h, bp_push_kernel, dim3(h->nw), dim3(128), 0, h->stream, h->xs, h->bp_hist, h->bp_n, h->bp_flag,
                       h->K, h->nbp);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_bp_fields(afq_handle *h, int i) {
    AFQ_LAUNCH(h, bp_fields_kernel, dim3(h->nw), dim3(128), 0, h->stream, h->bp_hist, h->bp_n, h->xs, h->alive,
                       h->K, h->nbp, i);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_bp_init(afq_handle *h, const cplx *phi0_dev) {
    const long per = (long)h->M * h->nt, n = per * h->nw;
    AFQ_LAUNCH(h, bp_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, phi0_dev, h->phi_bp,
                       per, h->nw);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_conj_copy(afq_handle *h, const cplx *src, cplx *dst, long n) {
    AFQ_LAUNCH(h, conj_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, src, dst, n);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_conj_transpose(afq_handle *h, const cplx *A, cplx *At) {
    AFQ_LAUNCH(h, conj_transpose_kernel, dim3((h->M * h->M + 255) / 256, 2), dim3(256), 0, h->stream, A, At,
                       h->M);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_bp_accumulate(afq_handle *h, int restore, int with_energy) {
    const long gsz = 2L * h->M * h->M;
    AFQ_LAUNCH(h, bp_accumulate_kernel, dim3((unsigned)((gsz + 4 + 127) / 128)), dim3(128), 0, h->stream, h->G,
                       h->weight, h->bp_cos, h->bp_ph, h->bp_est, h->nw, gsz, restore,
                       with_energy ? h->energy : (const cplx *)nullptr);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_bp_reset(afq_handle *h, bool first) {
    AFQ_LAUNCH(h, bp_reset_kernel, dim3((h->nw + 127) / 128), dim3(128), 0, h->stream, h->bp_n, h->bp_cos,
                       h->bp_ph, h->nw, (h->hirsch && !first) ? h->K : 0);
    AFQ_POST(h);
    return AFQ_OK;
}


int k_update_weight(afq_handle *h, cplx eshift) {
    const WeightArgs a = k_weight_args(h, eshift);
    AFQ_LAUNCH(h, weight_kernel, dim3((h->nw + 127) / 128), dim3(128), 0, h->stream, a);
    AFQ_POST(h);
    return AFQ_OK;
}

WeightArgs k_weight_args(afq_handle *h, cplx eshift) {
    WeightArgs a;
    a.nw = h->nw; a.flags = h->flags; a.dt = h->dt; a.eshift = eshift; a.alive = h->alive;
    a.ovlp_old = h->ovlp_old; a.ovlp_new = h->ovlp_new; a.cmf = h->cmf; a.cfb = h->cfb;
    a.weight = h->weight; a.ot = h->ot; a.ehyb = h->ehyb; a.phase = h->phase; a.counters = h->counters;
    a.eloc = h->eloc; a.energy = h->energy;
    a.bp_flag = h->nbp > 0 ? h->bp_flag : nullptr; a.bp_cos = h->bp_cos; a.bp_ph = h->bp_ph;
    a.cap_frac = h->cap_frac; a.cap_total = h->cap_total; a.cap_total_dev = h->scal;
    a.ot_scale = h->log_shift_on ? exp(-h->log_shift) : 1.0;
    a.est_acc = h->fuse_est_req ? h->est_acc : nullptr; a.unscaled = h->unscaled;
    return a;
}

// --------------------------------------------------------------------------
// Re-orthogonalisation: classical Gram-Schmidt applied twice per column.  With
// R_jj = ||v|| > 0 this is the unique QR with positive diagonal, i.e. exactly
// what the reference obtains from LAPACK QR followed by the sign fix
// (walkers/single_det.py:225-242); detR = prod_j R_jj over both spins.
struct QrArgs {
    int M, na, nb, nt, nw, in_lds, flags;
    cplx *phi;
    cplx *ws;           // global panel [nw, nmax, M] when it does not fit LDS
    double *detR, *weight;
    cplx *ot;
    const int *only;    // when set: redo only the walkers flagged by the Cholesky-QR path
    cplx *keep;         // cached overlap of a Green's function that stays valid across the QR (ovlp /= det R), or null
};

__global__ __launch_bounds__(NTHR) void reortho_kernel(QrArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ cplx coef[256];
    __shared__ double red[8];
    const int w = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (a.only && !a.only[w]) return;
    const int M = a.M, nt = a.nt;
    cplx *phi = a.phi + (long)w * M * nt;
    const int nmax = a.na > a.nb ? a.na : a.nb;
    cplx *Q = a.in_lds ? (cplx *)smem : a.ws + (long)w * nmax * M;     // Q[i][p], column i contiguous
    double logdet = 0.0;
    for (int s = 0; s < 2; ++s) {
        const int n = s == 0 ? a.na : a.nb, off = s == 0 ? 0 : a.na;
        if (n == 0) continue;
        for (int e = tid; e < n * M; e += NTHR) {
            const int p = e / n, i = e % n;
            Q[(long)i * M + p] = phi[(long)p * nt + off + i];
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            cplx *v = Q + (long)j * M;
            for (int pass = 0; pass < 2 && j > 0; ++pass) {
                for (int i = wave; i < j; i += NTHR / 64) {
                    const cplx *q = Q + (long)i * M;
                    double sr = 0, si = 0;
                    for (int p = lane; p < M; p += 64) {
                        const cplx x = q[p], y = v[p];      // conj(x) * y
                        sr += x.x * y.x + x.y * y.y;
                        si += x.x * y.y - x.y * y.x;
                    }
                    for (int o = 32; o > 0; o >>= 1) { sr += __shfl_down(sr, o); si += __shfl_down(si, o); }
                    if (lane == 0) coef[i] = cmake(sr, si);
                }
                __syncthreads();
                for (int p = tid; p < M; p += NTHR) {
                    cplx y = v[p];
                    for (int i = 0; i < j; ++i) {
                        const cplx c = coef[i], x = Q[(long)i * M + p];
                        y.x = fma(-c.x, x.x, y.x); y.x = fma(c.y, x.y, y.x);
                        y.y = fma(-c.x, x.y, y.y); y.y = fma(-c.y, x.x, y.y);
                    }
                    v[p] = y;
                }
                __syncthreads();
            }
            double nn = 0.0;
            for (int p = tid; p < M; p += NTHR) nn += cabs2(v[p]);
            nn = block_sum(nn, red);
            const double r = sqrt(nn), inv = 1.0 / r;
            logdet += log(r);
            for (int p = tid; p < M; p += NTHR) v[p] = cscale(v[p], inv);
            __syncthreads();
        }
        for (int e = tid; e < n * M; e += NTHR) {
            const int p = e / n, i = e % n;
            phi[(long)p * nt + off + i] = Q[(long)i * M + p];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double d = exp(logdet);
        a.detR[w] = d;
        a.ot[w] = cmake(a.ot[w].x / d, a.ot[w].y / d);           // single_det.py:253
        if (a.keep) a.keep[w] = cmake(a.keep[w].x / d, a.keep[w].y / d);
        if (a.flags & AFQ_PROP_FREE_PROJECTION) a.weight[w] *= d;  // walkers/handler.py:178-181
    }
}

// --------------------------------------------------------------------------
// Cholesky-QR2 of one walker in ONE work-group (N <= 32 electrons per spin, the walker and both Gram matrices in LDS).
// The GEMM-engine version (k_reortho_big: Gram, Cholesky, Q = phi R^-1 as three launches per pass, twice) spends
// ~160 us per re-orthogonalisation at C3 sizes on six latency-bound launches of 25 us each for ~5 us of arithmetic; here
// the passes run back to back out of LDS:
//   Gram  S_s = phi_s^H phi_s          fp64 MFMA, waves 0-3 spin up, 4-7 spin down, one 16x16 tile per wave
//   Chol  T = R^-1 (S = R^H R)         one wave per spin, register resident (chol_block8, gj_wave.h)
//   Q     phi_s <- phi_s T             fp64 MFMA, in place: a wave owns a 16-row tile, whose fragments it holds in registers
// Same algorithm, same fallback contract as k_reortho_big: a walker whose Cholesky breaks down (fail[w] = 1) is left
// untouched for the Gram-Schmidt kernel.  (reference: scipy.linalg.qr + sign fix, walkers/single_det.py:228-255)
#define RF_LD 33
struct RfArgs {
    int M, na, nb, nt, nw, fp;
    cplx *phi;
    double *detR, *weight;
    cplx *ot;
    int *fail;
    cplx *keep;          // cached overlap of a Green's function that stays valid across the QR (ovlp /= det R), or null
};

// RJ: registers per lane of the Cholesky wave (ceil(nmax / 2) rounded up to 4 / 8 / 13 / 16; one instantiation each: a kernel that
// carries all of them spills)
template <int RJ>
__global__ __launch_bounds__(512) void reortho_fused_kernel(RfArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ cplx rowk_s[2][32];
    __shared__ double piv_s[2][32];
    __shared__ double logd_s[2];
    __shared__ int bad_s[2];
    const int w = blockIdx.x, tid = threadIdx.x;
    const int g = __builtin_amdgcn_readfirstlane(tid >> 8), wave = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);
    const int lane = tid & 63, lr = lane & 15, lk = lane >> 4;
    const int M = a.M, nt = a.nt;
    const int n = g == 0 ? a.na : a.nb, off = g == 0 ? 0 : a.na;
    cplx *phi_l = (cplx *)smem;                              // [M, nt]
    cplx *S = phi_l + (long)M * nt + (long)g * (32 * RF_LD);   // [32, RF_LD] Gram matrix, then T^T, of this spin (row stride 33: no bank conflicts for a lane per row)
    cplx *phi_g = a.phi + (long)w * M * nt;
    {
        // the walker by LDS-DMA: 1 KB per wave and instruction, all requests of a wave in flight at once
        const unsigned total = (unsigned)(M * nt) * 16u;
        const int wave8 = __builtin_amdgcn_readfirstlane(tid >> 6);
        for (unsigned b0 = (unsigned)wave8 * 1024u; b0 < total; b0 += 8 * 1024u) {
            const unsigned bo = b0 + (unsigned)lane * 16u;
            if (bo < total) glds16((const char *)phi_g + bo, (char *)phi_l + b0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if (tid < 2) { logd_s[tid] = 0.0; bad_s[tid] = 0; }
    __syncthreads();
    const int nt16 = (n + 15) >> 4, mt16 = (M + 15) >> 4, nks = (M + 3) >> 2;
    for (int pass = 0; pass < 2; ++pass) {
        // ---- Gram matrix
        for (int t = wave; t < nt16 * nt16; t += 4) {
            const int ti = t / nt16, tj = t % nt16;
            const int ia = ti * 16 + lr, jb = tj * 16 + lr;
            const int iac = ia < n ? ia : n - 1, jbc = jb < n ? jb : n - 1;
            d4_t accR = {0, 0, 0, 0}, accI = {0, 0, 0, 0};
            // Rows / columns of the tile beyond n read a clamped (valid) column and produce numbers that are never stored: an
            // MFMA output element depends on its own A row and B column only.  Only the CONTRACTION index must not run past
            // M: whole steps of four are unconditional loads (no select for the compiler to turn into a branch around the
            // load), the last partial step selects.
            const cplx *xp = phi_l + lk * nt + off + iac, *yp = phi_l + lk * nt + off + jbc;
            const int nfull = M >> 2;
            // conj(x) * y by three multiplications: P1 = xr yr, P2 = xi yi, P3 = (xr - xi)(yr + yi); re = P1 + P2,
            // im = P3 - P1 + P2
            d4_t acc3 = {0, 0, 0, 0};
            // pairs of k-steps, the fragments of the next pair read from LDS ahead of the six MFMAs of this one (one k-step per
            // loop iteration put every pair of LDS reads directly in front of the MFMAs that wait for them)
            const int ngrp = nfull >> 1;
            cplx xa[2], ya[2], xb[2], yb[2];
            auto rd = [&](cplx (&x)[2], cplx (&y)[2], const int gq) __attribute__((always_inline)) {
#pragma unroll
                for (int u = 0; u < 2; ++u) { x[u] = xp[(gq * 2 + u) * 4 * nt]; y[u] = yp[(gq * 2 + u) * 4 * nt]; }
            };
            auto mf = [&](const cplx (&x)[2], const cplx (&y)[2]) __attribute__((always_inline)) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    accR = mfma16(x[u].x, y[u].x, accR);
                    accI = mfma16(x[u].y, y[u].y, accI);
                    acc3 = mfma16(x[u].x - x[u].y, y[u].x + y[u].y, acc3);
                }
            };
            if (ngrp > 0) rd(xa, ya, 0);
            for (int gq = 0; gq < ngrp; gq += 2) {
                if (gq + 1 < ngrp) rd(xb, yb, gq + 1);
                mf(xa, ya);
                if (gq + 1 < ngrp) {
                    if (gq + 2 < ngrp) rd(xa, ya, gq + 2);
                    mf(xb, yb);
                }
            }
            for (int ks = ngrp * 2; ks < nfull; ++ks) {
                const cplx x = xp[ks * 4 * nt], y = yp[ks * 4 * nt];
                accR = mfma16(x.x, y.x, accR);
                accI = mfma16(x.y, y.y, accI);
                acc3 = mfma16(x.x - x.y, y.x + y.y, acc3);
            }
            if (nfull < nks) {
                const int p = nfull * 4 + lk, pc = p < M ? p : M - 1;
                cplx x = phi_l[pc * nt + off + iac], y = phi_l[pc * nt + off + jbc];
                if (p >= M) { x = cmake(0.0, 0.0); y = cmake(0.0, 0.0); }
                accR = mfma16(x.x, y.x, accR);
                accI = mfma16(x.y, y.y, accI);
                acc3 = mfma16(x.x - x.y, y.x + y.y, acc3);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double p1 = accR[r], p2 = accI[r];
                accR[r] = p1 + p2; accI[r] = acc3[r] - p1 + p2;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = ti * 16 + lk + 4 * r, j = tj * 16 + lr;
                if (i < n && j < n) S[i * RF_LD + j] = cmake(accR[r], accI[r]);
            }
        }
        __syncthreads();
        // ---- inverse Cholesky factor: T^T[r][c] = conj(Ltilde^-1[r][c]) / sqrt(D_r) (see chol_small_kernel)
        if (wave == g && n > 0) {                            // (spin up on SIMD 0, spin down on SIMD 1: not both on one)
            bool bad = false;
            if (lane < 32) piv_s[g][lane] = 1.0;
            chol_wave_rj<RJ>(S, RF_LD, S, RF_LD, n, lane, rowk_s[g], piv_s[g], bad);
            double l = lane < n ? log(piv_s[g][lane & 31]) : 0.0;
            if (lane >= 32) l = 0.0;
            for (int o = 16; o > 0; o >>= 1) l += __shfl_down(l, o);
            // a pivot that is not a positive finite number: breakdown
            const unsigned long long anybad = __ballot(bad || !(l == l));
            if (lane == 0) {
                logd_s[g] += 0.5 * l;
                if (anybad) bad_s[g] = 1;
            }
        }
        __syncthreads();
        if (bad_s[0] | bad_s[1]) {                           // leave the walker to the Gram-Schmidt kernel
            if (tid == 0) a.fail[w] = 1;
            return;
        }
        // ---- Q = phi T in place: a wave takes whole 16-row tiles (all their columns), the row fragments in registers.
        // The fragments of T are the same for every row tile: read once per pass, all loads unconditional on clamped
        // indices (a clamped entry meets a zero of the row fragment or a column that is not stored), trip counts from RJ --
        // no branch between an LDS read and the MFMAs that wait for it.  T is upper triangular: the column tile j < 16
        // contracts k < 16 only.
        if (n > 0) {
            constexpr int KSN = (2 * RJ + 3) / 4 > 8 ? 8 : (2 * RJ + 3) / 4, TJN = 2 * RJ > 16 ? 2 : 1;
            cplx yf[TJN][KSN];
#pragma unroll
            for (int tj = 0; tj < TJN; ++tj)
#pragma unroll
                for (int ks = 0; ks < KSN; ++ks) {
                    const int k = ks * 4 + lk, kc = k < n ? k : n - 1;
                    const int jq = tj * 16 + lr, jc = jq < n ? jq : n - 1;
                    yf[tj][ks] = S[jc * RF_LD + kc];         // T[k][j] = T^T[j][k]
                }
            auto load_x = [&](cplx (&xf)[KSN], const int ti) __attribute__((always_inline)) {
                const int pa = ti * 16 + lr, pac = pa < M ? pa : M - 1;
#pragma unroll
                for (int ks = 0; ks < KSN; ++ks) {
                    const int k = ks * 4 + lk, kc = k < n ? k : n - 1;
                    const cplx x = phi_l[pac * nt + off + kc];
                    xf[ks] = (k < n && pa < M) ? x : cmake(0.0, 0.0);
                }
            };
            auto mul_store = [&](const cplx (&xf)[KSN], const int ti) __attribute__((always_inline)) {
                d4_t p1[TJN], p2[TJN], p3[TJN];
#pragma unroll
                for (int tj = 0; tj < TJN; ++tj) {
                    p1[tj] = (d4_t){0, 0, 0, 0}; p2[tj] = (d4_t){0, 0, 0, 0}; p3[tj] = (d4_t){0, 0, 0, 0};
                }
#pragma unroll
                for (int ks = 0; ks < KSN; ++ks) {
                    const cplx x = xf[ks];
                    const double xs = x.x + x.y;
#pragma unroll
                    for (int tj = 0; tj < TJN; ++tj) {
                        if (tj == 0 && TJN == 2 && ks >= 4) continue;      // (compile time) T[k][j] = 0 for k >= 16 > j
                        const cplx y = yf[tj][ks];
                        p1[tj] = mfma16(x.x, y.x, p1[tj]);
                        p2[tj] = mfma16(x.y, y.y, p2[tj]);
                        p3[tj] = mfma16(xs, y.x + y.y, p3[tj]);
                    }
                }
#pragma unroll
                for (int tj = 0; tj < TJN; ++tj) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int p = ti * 16 + lk + 4 * r, jq = tj * 16 + lr;
                        if (p < M && jq < n)
                            phi_l[p * nt + off + jq] = cmake(p1[tj][r] - p2[tj][r], p3[tj][r] - p1[tj][r] - p2[tj][r]);
                    }
                }
            };
            for (int ti = wave; ti < mt16; ti += 4) {
                cplx xa[KSN];
                load_x(xa, ti);
                mul_store(xa, ti);
            }
        }
        __syncthreads();
    }
    for (int e = tid; e < M * nt; e += 512) phi_g[e] = phi_l[e];
    if (tid == 0) {
        const double d = exp(logd_s[0] + logd_s[1]);
        a.fail[w] = 0;
        a.detR[w] = d;
        a.ot[w] = cmake(a.ot[w].x / d, a.ot[w].y / d);       // single_det.py:253
        if (a.keep) a.keep[w] = cmake(a.keep[w].x / d, a.keep[w].y / d);
        if (a.fp) a.weight[w] *= d;                          // walkers/handler.py:178-181
    }
}

static bool reortho_fused_supported(afq_handle *h, size_t *lds_out) {
    const int nmax = h->na > h->nb ? h->na : h->nb;
    const size_t lds = sizeof(cplx) * ((size_t)h->M * h->nt + 2 * 32 * RF_LD);
    *lds_out = lds;
    return nmax <= 32 && h->nb > 0 && h->M >= 16 && lds <= 150 * 1024;
}

static int k_reortho_fused(afq_handle *h, size_t lds, cplx *keep) {
    AFQ_TRY(dev_ensure(h, LT_WALKERS, &h->qr_fail, h->nw));
    RfArgs a;
    a.M = h->M; a.na = h->na; a.nb = h->nb; a.nt = h->nt; a.nw = h->nw;
    a.fp = (h->flags & AFQ_PROP_FREE_PROJECTION) ? 1 : 0;
    a.phi = h->phi; a.detR = h->detR; a.weight = h->weight; a.ot = h->ot; a.fail = h->qr_fail; a.keep = keep;
    const int nmax_rj = h->na > h->nb ? h->na : h->nb;
    const int rji = nmax_rj <= 8 ? 0 : nmax_rj <= 16 ? 1 : nmax_rj <= 26 ? 2 : 3;
    const void *kfn[4] = {(const void *)reortho_fused_kernel<4>, (const void *)reortho_fused_kernel<8>,
                          (const void *)reortho_fused_kernel<13>, (const void *)reortho_fused_kernel<16>};
    static size_t lds_set4[4][AFQ_MAX_DEVICES] = {{0}};
    AFQ_HIP(h, afq_raise_lds(kfn[rji], lds, lds_set4[rji]));
    if (rji == 0) AFQ_LAUNCH(h, reortho_fused_kernel<4>, dim3(h->nw), dim3(512), lds, h->stream, a);
    else if (rji == 1) AFQ_LAUNCH(h, reortho_fused_kernel<8>, dim3(h->nw), dim3(512), lds, h->stream, a);
    else if (rji == 2) AFQ_LAUNCH(h, reortho_fused_kernel<13>, dim3(h->nw), dim3(512), lds, h->stream, a);
    else AFQ_LAUNCH(h, reortho_fused_kernel<16>, dim3(h->nw), dim3(512), lds, h->stream, a);
    AFQ_POST(h);
    return AFQ_OK;
}

// keep: the cached overlap to divide by det R along the way (null: none).  *keep_done tells the caller whether the kernels
// did that (fused Cholesky-QR path and its Gram-Schmidt fallback) or a separate pass is still due.
int k_reortho(afq_handle *h, cplx *keep, bool *keep_done) {
    QrArgs a;
    a.M = h->M; a.na = h->na; a.nb = h->nb; a.nt = h->nt; a.nw = h->nw; a.flags = h->flags;
    a.phi = h->phi; a.detR = h->detR; a.weight = h->weight; a.ot = h->ot;
    a.only = nullptr; a.keep = nullptr;
    if (keep_done) *keep_done = false;
    const int nmax = h->na > h->nb ? h->na : h->nb;
    // Cholesky-QR2 on the GEMM engines: always for 45 < N <= 128; for smaller N once the population is
    // large enough that seven launches beat the one latency-bound Gram-Schmidt work-group per walker
    const bool small_ok = nmax <= 45 && h->nb > 0 && h->nw >= 64 && h->M >= 32;
    size_t lds_fused = 0;
    if (small_ok && reortho_fused_supported(h, &lds_fused)) {
        int rc = k_reortho_fused(h, lds_fused, keep);
        if (rc) return rc;
        a.only = h->qr_fail; a.keep = keep;
        if (keep_done) *keep_done = keep != nullptr;
    } else if (k_greens_big_supported(h) || small_ok) {
        int rc = k_reortho_big(h);
        if (rc) return rc;
        a.only = h->qr_fail;
    }
    const size_t need = sizeof(cplx) * (size_t)nmax * h->M;
    a.in_lds = need <= 64 * 1024;
    a.ws = h->phi_t2;       // scratch panel (nmax*M <= M*nt elements per walker)
    AFQ_LAUNCH(h, reortho_kernel, dim3(h->nw), dim3(NTHR), a.in_lds ? need : 0, h->stream, a);
    AFQ_POST(h);
    return AFQ_OK;
}

// --------------------------------------------------------------------------
__global__ void cap_kernel(double *weight, int nw, double cap) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w < nw && fabs(weight[w]) > cap) weight[w] = cap;       // qmc/afqmc.py:235-236
}

__global__ void cap_dev_kernel(double *weight, int nw, double frac, const double *scal) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    const double cap = frac * scal[0];                          // total weight of the last comb
    if (w < nw && fabs(weight[w]) > cap) weight[w] = cap;
}

int k_cap_weights(afq_handle *h, double frac, double total_weight) {
    if (total_weight < 0.0) {
        AFQ_LAUNCH(h, cap_dev_kernel, dim3((h->nw + 255) / 256), dim3(256), 0, h->stream, h->weight, h->nw,
                           frac, h->scal);
        AFQ_POST(h);
        return AFQ_OK;
    }
    AFQ_LAUNCH(h, cap_kernel, dim3((h->nw + 255) / 256), dim3(256), 0, h->stream, h->weight, h->nw,
                       frac * total_weight);
    AFQ_POST(h);
    return AFQ_OK;
}

__global__ void scale_kernel(double *weight, double *unscaled, int nw, double scale) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w < nw) { unscaled[w] = weight[w]; weight[w] = weight[w] / scale; }   // handler.py:244-246
}

int k_scale_weights(afq_handle *h, double scale) {
    AFQ_LAUNCH(h, scale_kernel, dim3((h->nw + 255) / 256), dim3(256), 0, h->stream, h->weight,
                       h->unscaled, h->nw, scale);
    AFQ_POST(h);
    return AFQ_OK;
}

__global__ void reset_kernel(double *weight, int nw, const double *scal) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (scal && scal[1] < 0.0) return;                             // collapsed population: see comb_plan_kernel
    if (w < nw) weight[w] = 1.0;                                   // handler.py:337-338
}

int k_reset_weights(afq_handle *h, bool after_comb) {
    AFQ_LAUNCH(h, reset_kernel, dim3((h->nw + 255) / 256), dim3(256), 0, h->stream, h->weight, h->nw,
               after_comb ? (const double *)h->scal : (const double *)nullptr);
    AFQ_POST(h);
    return AFQ_OK;
}

// Single-rank comb (walkers/handler.py:225-301).  The cumulative sums and the
// walk over the comb teeth are inherently sequential and must reproduce the
// reference's left-to-right double additions, so one thread does them (nw adds).
// scal[0] = total weight (before scaling), scal[1] = number of (clone, kill) pairs.
// Comb population control, walkers/handler.py:225-338, decided by one work-group: every thread owns a
// contiguous chunk of walkers (sequential sums inside the chunk, prefix scans across chunks), every
// comb tooth is located in the cumulative weights by bisection, and the clone / kill lists are
// compacted with prefix counts so that the j-th walker with multiplicity > 1 overwrites the j-th walker
// with multiplicity 0 -- exactly the zip(clone, kill) pairing (one copy per parent, :295-301).
__global__ __launch_bounds__(256) void comb_plan_kernel(double *weight, double *unscaled, int nw, double r,
                                                         double target, int *parent_ix, int *pairs,
                                                         double *scal) {
    extern __shared__ __align__(16) unsigned char smem[];
    double *cs = (double *)smem;              // |w| / scale, then its inclusive cumulative sum
    int *pix = (int *)(cs + nw);
    int *clone_l = pix + nw, *kill_l = clone_l + nw;
    __shared__ double wtot_d[4];
    __shared__ int wtot_i[4];
    const int tid = threadIdx.x;
    const int per = (nw + 255) / 256;
    const int i0 = tid * per < nw ? tid * per : nw, i1 = (tid + 1) * per < nw ? (tid + 1) * per : nw;
    double loc = 0.0;
    for (int i = i0; i < i1; ++i) { const double a = fabs(weight[i]); cs[i] = a; pix[i] = 0; loc += a; }
    double total;
    (void)block_excl_scan256(loc, wtot_d, &total);            // sum(global_weights), handler.py:233
    if (tid == 0) scal[0] = total;
    // handler.py:236-241: the reference stops here.  Nothing is cloned, the weights are left alone, and the sticky
    // flag scal[2] makes the next synchronising call (afq_popcontrol_comb with outputs, afq_estimates_get)
    // return AFQ_EWEIGHT
    if (total < 1e-8) { if (tid == 0) { scal[1] = -1.0; scal[2] = 1.0; } return; }
    const double scale = total / target;
    loc = 0.0;
    for (int i = i0; i < i1; ++i) {
        unscaled[i] = weight[i];                              // handler.py:245
        weight[i] = weight[i] / scale;
        const double a = cs[i] / scale;                       // global_weights / scale, handler.py:248
        loc += a;
        cs[i] = loc;                                          // chunk-local running sum
    }
    double tot2;
    const double base = block_excl_scan256(loc, wtot_d, &tot2);   // sum(weights), handler.py:274
    for (int i = i0; i < i1; ++i) cs[i] += base;              // numpy.cumsum(weights)
    __syncthreads();
    const int ntarget = (int)target;
    const double step = tot2 / target;
    for (int ic = tid; ic < ntarget; ic += 256) {
        const double tooth = (ic + r) * step;
        int lo = 0, hi = nw;                                  // smallest iw with tooth < cs[iw]
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (tooth < cs[mid]) hi = mid; else lo = mid + 1;
        }
        if (lo < nw) atomicAdd(&pix[lo], 1);
    }
    __syncthreads();
    int nc = 0, nk = 0;
    for (int i = i0; i < i1; ++i) { nc += pix[i] > 1; nk += pix[i] == 0; }
    int totc, totk;
    int bc = block_excl_scan256(nc, wtot_i, &totc);
    int bk = block_excl_scan256(nk, wtot_i, &totk);
    for (int i = i0; i < i1; ++i) {
        if (pix[i] > 1) clone_l[bc++] = i;
        if (pix[i] == 0) kill_l[bk++] = i;
        parent_ix[i] = pix[i];
    }
    __syncthreads();
    const int np = totc < totk ? totc : totk;
    for (int j = tid; j < np; j += 256) { pairs[2 * j] = clone_l[j]; pairs[2 * j + 1] = kill_l[j]; }
    if (tid == 0) scal[1] = (double)np;
}

struct CloneArgs {
    WalkerFields f;      // what travels with a walker (walker_fields.h), never the weight
    const int *pairs;
    const double *scal;
    double *weight;      // single-rank comb: every weight back to 1 (handler.py:337-338) in this launch; null otherwise
    int nw;
};

__global__ void clone_kernel(CloneArgs a) {
    const int pr = blockIdx.y;
    if (a.weight && blockIdx.x == 0 && !(a.scal[1] < 0.0)) {        // (collapsed population: see comb_plan_kernel)
        const int wr = blockIdx.y * blockDim.x + threadIdx.x;
        if (wr < a.nw) a.weight[wr] = 1.0;
    }
    if (pr >= (int)a.scal[1]) return;
    const long src = a.pairs[2 * pr], dst = a.pairs[2 * pr + 1];
    const long t0 = blockIdx.x * (long)blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
    for (int k = 0; k < a.f.n; ++k) {
        const WalkerFields::Entry e = a.f.e[k];
        walker_field_copy(e.base + dst * e.bytes, e.base + src * e.bytes, e.bytes, t0, stride);
    }
}

__global__ void scale_by_inverse_kernel(cplx *x, const double *d, int nw) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w < nw) x[w] = cmake(x[w].x / d[w], x[w].y / d[w]);
}

// use_log_shift, walkers/single_det.py:250-253 on top of the plain QR bookkeeping the re-orthogonalisation kernels
// leave behind (detR = det R, ot /= det R, free projection: weight *= det R):
// detR -> exp(log det R - detR_shift), ot and the free-projection weight follow, log_detR += log(detR).
__global__ void log_shift_reortho_kernel(cplx *ot, double *detR, double *weight, double *log_detR, int nw,
                                         double detR_shift, int fp) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    const double raw = detR[w], d = exp(log(raw) - detR_shift), f = raw / d;
    detR[w] = d;
    ot[w] = cscale(ot[w], f);
    if (fp) weight[w] /= f;
    log_detR[w] += log(d);
}

int k_log_shift_reortho(afq_handle *h) {
    AFQ_LAUNCH(h, log_shift_reortho_kernel, dim3((h->nw + 127) / 128), dim3(128), 0, h->stream, h->ot, h->detR,
               h->weight, h->log_detR, h->nw, h->detR_shift, (h->flags & AFQ_PROP_FREE_PROJECTION) ? 1 : 0);
    AFQ_POST(h);
    return AFQ_OK;
}

// walkers/handler.py:457-462: sums of |ot|, |detR|, |log_detR| over this rank's walkers, one work-group
__global__ __launch_bounds__(256) void log_ovlp_sums_kernel(const cplx *ot, const double *detR, const double *log_detR,
                                                            int nw, double *out) {
    __shared__ double red[3][256];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int w = threadIdx.x; w < nw; w += 256) {
        s0 += hypot(ot[w].x, ot[w].y); s1 += fabs(detR[w]); s2 += fabs(log_detR[w]);
    }
    red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x < 3) out[threadIdx.x] = red[threadIdx.x][0];
}

int k_log_ovlp_sums(afq_handle *h, double *out3) {
    double *tmp = (double *)h->pack_tmp;
    AFQ_LAUNCH(h, log_ovlp_sums_kernel, dim3(1), dim3(256), 0, h->stream, h->ot, h->detR, h->log_detR, h->nw, tmp);
    AFQ_POST(h);
    AFQ_HIP(h, hipMemcpyAsync(out3, tmp, 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    AFQ_HIP(h, hipStreamSynchronize(h->stream));
    return AFQ_OK;
}

int k_scale_by_inverse(afq_handle *h, cplx *x, const double *d) {
    AFQ_LAUNCH(h, scale_by_inverse_kernel, dim3((h->nw + 127) / 128), dim3(128), 0, h->stream, x, d, h->nw);
    AFQ_POST(h);
    return AFQ_OK;
}

// clone_kernel over the (src, dst) pairs in h->pack_tmp, count in scal[1]; at most nw / 2 pairs
int k_clone_pairs(afq_handle *h, bool with_greens, bool reset_weights) {
    // cloned walkers bring their Ghalf along, and its spin sum when that is current (it then stays current)
    // the clone kernel copies whole walkers with Ghalf, its spin sum and the diagonal sums, and a copy of a closed-shell
    // walker is one: everything derived stays current
    const bool sum_too = with_greens && h->gf.gsum.current(h->gf), diag_too = with_greens && h->gf.gdiag.current(h->gf);
    h->gf.cloned(with_greens ? GreensCache::SUM | GreensCache::DIAG | GreensCache::CLOSED : 0);
    CloneArgs a;
    a.f = walker_fields(h, (with_greens ? WF_GREENS : 0) | (sum_too ? WF_GSUM : 0) | (diag_too ? WF_GDIAG : 0));
    a.pairs = (const int *)h->pack_tmp; a.scal = h->scal;
    a.weight = reset_weights ? h->weight : nullptr; a.nw = h->nw;
    // (grid.y * 256 threads of the x == 0 blocks cover every walker for the weight reset)
    AFQ_LAUNCH(h, clone_kernel, dim3(4, (h->nw + 1) / 2), dim3(256), 0, h->stream, a);
    AFQ_POST(h);
    return AFQ_OK;
}

// ---- closed-shell walkers on the large-system path (afq_internal.h: closed_large) ----
// one work-group per walker: are the alpha and the beta block bitwise equal?  (na == nb)
__global__ __launch_bounds__(256) void closed_flags_kernel(const cplx *phi, int M, int na, int nt, const int *alive, int *flags,
                                                           unsigned long long *counters) {
    const int w = blockIdx.x;
    if (alive && !alive[w]) { if (threadIdx.x == 0) flags[w] = 0; return; }
    const cplx *p = phi + (long)w * M * nt;
    int same = 1;
    for (int e = threadIdx.x; e < M * na; e += 256) {
        const int r = e / na, c = e - r * na;
        const cplx x = p[r * nt + c], y = p[r * nt + na + c];
        same &= (int)((__double_as_longlong(x.x) == __double_as_longlong(y.x)) & (__double_as_longlong(x.y) == __double_as_longlong(y.y)));
    }
    const int all = __syncthreads_and(same);
    if (threadIdx.x == 0) {
        flags[w] = all ? 1 : 0;
        if (all && counters) atomicAdd(&counters[7], 1ull);       // afq_counters_ext [7]
    }
}

__global__ __launch_bounds__(256) void closed_copy_beta_kernel(cplx *phi, int M, int na, int nt, const int *flags) {
    const int w = blockIdx.x;
    if (!flags[w]) return;
    cplx *p = phi + (long)w * M * nt;
    for (int e = threadIdx.x; e < M * na; e += 256) {
        const int r = e / na, c = e - r * na;
        p[r * nt + na + c] = p[r * nt + c];
    }
}

int k_closed_flags(afq_handle *h) {
    AFQ_TRY(dev_grow(h, LT_WALKERS, &h->closed_w, &h->closed_w_n, (size_t)h->nw, "closed-shell flags"));
    AFQ_LAUNCH(h, closed_flags_kernel, dim3(h->nw), dim3(256), 0, h->stream, h->phi, h->M, h->na, h->nt, h->alive, h->closed_w, h->counters);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_closed_copy_beta(afq_handle *h) {

    AFQ_LAUNCH(h, closed_copy_beta_kernel, dim3(h->nw), dim3(256), 0, h->stream, h->phi, h->M, h->na, h->nt, h->closed_w);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_comb(afq_handle *h, double r, double target, bool with_greens) {
    if (k_comm_size(h) > 1 || h->comm) return k_comm_popcontrol(h, r, target, with_greens);
    int *pairs = (int *)h->pack_tmp;
    AFQ_LAUNCH(h, comb_plan_kernel, dim3(1), dim3(256), (sizeof(double) + 3 * sizeof(int)) * (size_t)h->nw,
               h->stream, h->weight, h->unscaled, h->nw, r, target, h->parent_ix, pairs, h->scal);
    AFQ_POST(h);
    return k_clone_pairs(h, with_greens, true);       // the weights go back to 1 in the same launch
}

// Pair-branch population control, walkers/handler.py:225-251,340-412, decided by one work-group.
//   total, scaling   as comb_plan_kernel (the same chunked sums), scal[0] = total, collapsed population: same exit
//   sort             a_i = |weight_i / scale| ascending and stable (argsort(kind='mergesort'), :348): a bitonic network
//                    in LDS on the composite key (a_i, i), padded to a power of two with (+inf, index >= nw) keys --
//                    data independent, so it terminates whatever the weights are
//   pairs            pair p = (sorted[p], sorted[nw-1-p]) is acted on while every earlier pair was and
//                    a_s < min_weight or a_e > max_weight (:356, :385-386); it reads u[p], its one uniform (:359), and
//                    the walker it clones gets 0.5 * (a_s + a_e) (:362, :373).  "Every earlier pair was" is the index
//                    of the first pair that fails the test: a minimum over the pairs (atomicMin on one LDS word, the
//                    same value in whatever order the threads arrive), not a prefix scan of flags
//   placement        clones and kills compacted by index, the j-th clone overwrites the j-th kill (all of :396-410's
//                    messages carry the same tag on one rank); the killed slot gets the weight of the clone that lands
//                    there, which clone_kernel does not copy
// Out: parent_ix[i] = 0 kill / 1 keep / 2 clone, pairs for clone_kernel, scal[1] = pairs, scal[9] = uniforms consumed.
// LDS: P * 12 + nw * 4 bytes for P = nw rounded up to a power of two; the clone / kill lists reuse the sort keys.
__global__ __launch_bounds__(256) void pair_branch_plan_kernel(double *weight, double *unscaled, int nw, int P,
                                                                const double *u, double target, double min_weight,
                                                                double max_weight, int *parent_ix, int *pairs,
                                                                double *scal) {
    extern __shared__ __align__(16) unsigned char smem[];
    double *key = (double *)smem;             // [P] a_i, sorted
    int *idx = (int *)(key + P);              // [P] walker of each sorted position
    int *mult = idx + P;                      // [nw]
    __shared__ double wtot_d[4];
    __shared__ int wtot_i[4];
    __shared__ int s_first;                   // first pair that is not acted on
    const int tid = threadIdx.x;
    const int per = (nw + 255) / 256;
    const int i0 = tid * per < nw ? tid * per : nw, i1 = (tid + 1) * per < nw ? (tid + 1) * per : nw;
    double loc = 0.0;
    for (int i = i0; i < i1; ++i) loc += fabs(weight[i]);
    double total;
    (void)block_excl_scan256(loc, wtot_d, &total);            // sum(global_weights), handler.py:233
    if (tid == 0) scal[0] = total;
    if (total < 1e-8) { if (tid == 0) { scal[1] = -1.0; scal[2] = 1.0; } return; }      // handler.py:236-241
    const double scale = total / target;
    for (int i = i0; i < i1; ++i) {
        unscaled[i] = weight[i];                              // handler.py:245
        const double w = weight[i] / scale;
        weight[i] = w;
        key[i] = fabs(w);                                     // handler.py:341
        idx[i] = i;
        mult[i] = 1;
    }
    for (int i = nw + tid; i < P; i += 256) { key[i] = INFINITY; idx[i] = i; }
    if (tid == 0) s_first = nw / 2;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += 256) {
                const int lo = 2 * t - (t & (j - 1)), hi = lo + j;        // the two positions that differ in bit j
                const double ka = key[lo], kb = key[hi];
                const int ia = idx[lo], ib = idx[hi];
                const bool a_after_b = ka > kb || (ka == kb && ia > ib);
                if (a_after_b == ((lo & k) == 0)) { key[lo] = kb; key[hi] = ka; idx[lo] = ib; idx[hi] = ia; }
            }
            __syncthreads();
        }
    }
    const int npairs = nw / 2;
    for (int p = tid; p < npairs; p += 256) {
        const int is = idx[p], ie = idx[nw - 1 - p];
        // (a padding key among the first nw positions can only follow from NaN weights: never index with it)
        if (!(key[p] < min_weight || key[nw - 1 - p] > max_weight) || is >= nw || ie >= nw) { atomicMin(&s_first, p); break; }
    }
    __syncthreads();
    const int nact = s_first;
    for (int p = tid; p < nact; p += 256) {
        const int is = idx[p], ie = idx[nw - 1 - p];
        const double a_s = key[p], a_e = key[nw - 1 - p];
        const double wab = a_s + a_e;                         // handler.py:358
        const bool big = u[p] < a_e / wab;                    // handler.py:360
        const int clone = big ? ie : is, kill = big ? is : ie;
        weight[clone] = 0.5 * wab;                            // handler.py:362,373
        mult[clone] = 2; mult[kill] = 0;
    }
    __syncthreads();                                          // (the keys are dead from here: their LDS holds the lists)
    int *clone_l = (int *)key, *kill_l = clone_l + nw;
    int nc = 0, nk = 0;
    for (int i = i0; i < i1; ++i) { nc += mult[i] == 2; nk += mult[i] == 0; }
    int totc, totk;
    int bc = block_excl_scan256(nc, wtot_i, &totc);
    int bk = block_excl_scan256(nk, wtot_i, &totk);
    for (int i = i0; i < i1; ++i) {
        if (mult[i] == 2) clone_l[bc++] = i;
        if (mult[i] == 0) kill_l[bk++] = i;
        parent_ix[i] = mult[i];
    }
    __syncthreads();
    const int np = totc < totk ? totc : totk;                 // (both equal nact)
    for (int j = tid; j < np; j += 256) {
        pairs[2 * j] = clone_l[j]; pairs[2 * j + 1] = kill_l[j];
        weight[kill_l[j]] = weight[clone_l[j]];               // the buffer that travels holds the new weight, handler.py:399-410
    }
    if (tid == 0) { scal[1] = (double)np; scal[9] = (double)nact; }
}

int k_pair_branch(afq_handle *h, const double *u_dev, double target, double min_weight, double max_weight,
                  bool with_greens) {
    if (h->nw > AFQ_PAIR_BRANCH_MAX_WALKERS)
        AFQ_FAIL(h, AFQ_EUNSUPPORTED, "pair branching on the device serves at most AFQ_PAIR_BRANCH_MAX_WALKERS (8192) walkers per handle");
    int P = 2;
    while (P < h->nw) P <<= 1;
    const size_t lds = (sizeof(double) + sizeof(int)) * (size_t)P + sizeof(int) * (size_t)h->nw;
    static size_t lds_set[AFQ_MAX_DEVICES] = {0};
    // (the default limit of 64 KiB covers the kernel's few static words too: 4096 walkers are already above it)
    if (lds + 256 > 64 * 1024) AFQ_HIP(h, afq_raise_lds((const void *)pair_branch_plan_kernel, lds, lds_set));
    AFQ_LAUNCH(h, pair_branch_plan_kernel, dim3(1), dim3(256), lds, h->stream, h->weight, h->unscaled, h->nw, P, u_dev,
               target, min_weight, max_weight, h->parent_ix, (int *)h->pack_tmp, h->scal);
    AFQ_POST(h);
    return k_clone_pairs(h, with_greens, false);      // nothing is reset: the plan has written both weights
}

// --------------------------------------------------------------------------
// estimators/mixed.py:211-225: one workgroup, deterministic tree sums.
// estimators/mixed.py:151-175, 211-225: one workgroup, deterministic tree sums.
__global__ __launch_bounds__(NTHR) void estimates_kernel(int nw, int have_energy, int fp, const double *weight,
                                                         const double *unscaled, const cplx *ot,
                                                         const cplx *ehyb, const cplx *phase, const cplx *energy,
                                                         cplx *est, double *acc, int fold_only, EstPublish pub) {
    __shared__ double red[NTHR / 64][18];
    // v[0]=uweight  v[1..2]=weight  v[3]=ovlp  v[4..5]=ehyb  v[6..7]=enumer  v[8..9]=e1b  v[10..11]=e2b
    // v[12..17] = the first six again for the steps whose sums rode on their weight update (afq_estimates_fuse_next):
    // kept apart, the energy denominator of THIS step is this step's weight sum only
    double v[18];
    for (int k = 0; k < 18; ++k) v[k] = 0.0;
    for (int w = threadIdx.x; w < nw; w += NTHR) {
        if (acc) {       // fold and clear
#pragma unroll
            for (int k = 0; k < 6; ++k) { v[12 + k] += acc[6 * w + k]; acc[6 * w + k] = 0.0; }
        }
        if (fold_only) continue;
        const double x = weight[w];
        // importance sampling: wfac = weight (mixed.py:217-225); free projection: weight*ot*phase (:154)
        cplx wf = cmake(x, 0.0);
        if (fp) wf = cscale(cmul(ot[w], phase[w]), x);
        v[0] += unscaled[w];
        v[1] += wf.x; v[2] += wf.y;
        v[3] += x * hypot(ot[w].x, ot[w].y);
        const cplx eh = cmul(wf, ehyb[w]);
        v[4] += eh.x; v[5] += eh.y;
        if (have_energy) {
            if (fp) {
                const cplx e0 = cmul(wf, energy[3 * w]), e1 = cmul(wf, energy[3 * w + 1]), e2 = cmul(wf, energy[3 * w + 2]);
                v[6] += e0.x; v[7] += e0.y; v[8] += e1.x; v[9] += e1.y; v[10] += e2.x; v[11] += e2.y;
            } else {
                v[6] += x * energy[3 * w].x; v[8] += x * energy[3 * w + 1].x; v[10] += x * energy[3 * w + 2].x;
            }
        }
    }
    // all sums in one pass: wave shuffles, one barrier, thread 0 adds the per-wave partials in wave order
    const int nk = have_energy ? 12 : 6;                     // the energy sums stay zero (and unused) on the other steps
#pragma unroll
    for (int k = 0; k < 18; ++k)
        if (k < nk || (k >= 12 && acc))
            for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 18; ++k) red[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 18; ++k) {
            v[k] = 0.0;
            for (int i = 0; i < NTHR / 64; ++i) v[k] += red[i][k];
        }
        est[AFQ_EST_UWEIGHT].x += v[0] + v[12];
        est[AFQ_EST_WEIGHT].x += v[1] + v[13]; est[AFQ_EST_WEIGHT].y += v[2] + v[14];
        est[AFQ_EST_OVLP].x += v[3] + v[15];
        est[AFQ_EST_EHYB].x += v[4] + v[16]; est[AFQ_EST_EHYB].y += v[5] + v[17];
        if (have_energy) {
            est[AFQ_EST_ENUMER].x += v[6]; est[AFQ_EST_ENUMER].y += v[7];
            est[AFQ_EST_E1B].x += v[8]; est[AFQ_EST_E1B].y += v[9];
            est[AFQ_EST_E2B].x += v[10]; est[AFQ_EST_E2B].y += v[11];
            est[AFQ_EST_EDENOM].x += v[1]; est[AFQ_EST_EDENOM].y += v[2];
        }
    }
    if (pub.host_out) {
        // the block's sums go to the host from this launch (afq_api.hip: est_publish_kernel, the same steps): one launch less
        // at every block boundary
        __syncthreads();                                 // thread 0's sums, for the threads that copy them out
        const int t = threadIdx.x;
        if (t < pub.nest) pub.host_out[t] = ((const double *)est)[t];
        if (t < AFQ_NSCAL) pub.host_out[pub.nest + t] = pub.scal[t];
        if (t == 0) pub.host_seq[1] = pub.closed_bad ? *pub.closed_bad : 0ull;
        __threadfence_system();
        __syncthreads();
        if (t < pub.nest && pub.zero) ((double *)est)[t] = 0.0;
        if (t == 0) __hip_atomic_store(pub.host_seq, pub.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// estimators/mixed.py:226-229: estimates[one_rdm] += weight * walker.G.real, summed over walkers in a fixed order
__global__ void rdm_accumulate_kernel(const cplx *G, const double *weight, double *acc, int nw, long gsz) {
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (e >= gsz) return;
    double s = 0.0;
    for (int w = 0; w < nw; ++w) s = fma(weight[w], G[(long)w * gsz + e].x, s);
    acc[e] += s;
}

int k_rdm_accumulate(afq_handle *h) {
    const long gsz = 2L * h->M * h->M;
    AFQ_LAUNCH(h, rdm_accumulate_kernel, dim3((unsigned)((gsz + 127) / 128)), dim3(128), 0, h->stream, h->G, h->weight,
               h->rdm_acc, h->nw, gsz);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_estimates(afq_handle *h, int have_energy, bool fold_only, const EstPublish *pub) {
    const int fp = (h->flags & AFQ_PROP_FREE_PROJECTION) ? 1 : 0;
    if (fold_only && !h->est_acc_pending) return AFQ_OK;
    AFQ_LAUNCH(h, estimates_kernel, dim3(1), dim3(NTHR), 0, h->stream, h->nw, have_energy, fp, h->weight,
                       h->unscaled, h->ot, h->ehyb, h->phase, h->energy, h->estimates,
                       h->est_acc_pending ? h->est_acc : (double *)nullptr, fold_only ? 1 : 0, pub ? *pub : EstPublish());
    AFQ_POST(h);
    h->est_acc_pending = false;
    return AFQ_OK;
}

// also refreshes the alive flags of the step (qmc/afqmc.py:232) so that the device-RNG path needs no
// separate alive_kernel launch
__global__ void rng_normal_kernel(double *xi, long n, unsigned long long seed, unsigned long long stream,
                                  unsigned long long counter, const double *weight, int *alive, int nw) {
    const long pair = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (pair < nw) alive[pair] = fabs(weight[pair]) > 1e-8 ? 1 : 0;
    if (2 * pair >= n) return;
    double x0, x1;
    philox_normal_pair(pair, seed, stream, counter, x0, x1);
    xi[2 * pair] = x0;
    if (2 * pair + 1 < n) xi[2 * pair + 1] = x1;
}

// uniforms in [0, 1) (53 bits), same counter-based stream
__global__ void rng_uniform_kernel(double *u, long n, unsigned long long seed, unsigned long long stream,
                                   unsigned long long counter) {
    const long pair = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (2 * pair >= n) return;
    unsigned int c0 = (unsigned int)pair, c1 = (unsigned int)(pair >> 32);
    unsigned int c2 = (unsigned int)counter, c3 = (unsigned int)(counter >> 32) ^ (unsigned int)(stream * 0x9E3779B9u);
    unsigned int k0 = (unsigned int)seed, k1 = (unsigned int)(seed >> 32);
    for (int rd = 0; rd < 10; ++rd) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const unsigned long long a = (((unsigned long long)c0 << 32) | c1) >> 11;
    const unsigned long long b = (((unsigned long long)c2 << 32) | c3) >> 11;
    u[2 * pair] = (double)a * (1.0 / 9007199254740992.0);
    if (2 * pair + 1 < n) u[2 * pair + 1] = (double)b * (1.0 / 9007199254740992.0);
}

int k_rng_uniform(afq_handle *h, double *u, long n) {
    const long pairs = (n + 1) / 2;
    AFQ_LAUNCH(h, rng_uniform_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, h->stream, u, n,
                       (unsigned long long)h->rng_seed, (unsigned long long)h->rng_stream,
                       (unsigned long long)h->rng_counter);
    AFQ_POST(h);
    h->rng_counter += 1;
    return AFQ_OK;
}

// test hooks (afq_rng_normal / afq_rng_philox4x32): the same stream into a caller-provided device buffer, and
// the bare Philox4x32-10 block function for the Random123 known-answer vectors
int k_rng_normal_into(afq_handle *h, double *out_d, long n) {
    const long pairs = (n + 1) / 2;
    AFQ_LAUNCH(h, rng_normal_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, h->stream, out_d, n,
               (unsigned long long)h->rng_seed, (unsigned long long)h->rng_stream,
               (unsigned long long)h->rng_counter, (const double *)nullptr, (int *)nullptr, 0);
    AFQ_POST(h);
    h->rng_counter += 1;
    return AFQ_OK;
}

__global__ void philox_raw_kernel(const unsigned int *in, unsigned int *out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned int c0 = in[6 * i], c1 = in[6 * i + 1], c2 = in[6 * i + 2], c3 = in[6 * i + 3];
    unsigned int k0 = in[6 * i + 4], k1 = in[6 * i + 5];
    for (int rd = 0; rd < 10; ++rd) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[4 * i] = c0; out[4 * i + 1] = c1; out[4 * i + 2] = c2; out[4 * i + 3] = c3;
}

int k_philox_raw(afq_handle *h, const unsigned int *in_d, unsigned int *out_d, int n) {
    AFQ_LAUNCH(h, philox_raw_kernel, dim3((n + 63) / 64), dim3(64), 0, h->stream, in_d, out_d, n);
    AFQ_POST(h);
    return AFQ_OK;
}

int k_rng_normal(afq_handle *h) {
    const long n = (long)h->nw * h->K;
    const long pairs = std::max((n + 1) / 2, (long)h->nw);
    AFQ_LAUNCH(h, rng_normal_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, h->stream, h->xi, n,
                       (unsigned long long)h->rng_seed, (unsigned long long)h->rng_stream,
                       (unsigned long long)h->rng_counter, h->weight, h->alive, h->nw);
    AFQ_POST(h);
    h->rng_counter += 1;
    return AFQ_OK;
}
