// Green's function / overlap of one walker with at most 45 electrons per spin, as device code: the body of
// greens_small_kernel (k_small.hip), which the fused propagator (k_fused.hip) also runs as the tail of its own launch on the
// steps afq_set_step_fusion_scope names -- one work-group of 512 threads per walker in both, the same code and the same bits.
#pragma once
#include <type_traits>
#include "mfma_gemm.h"
#include "gj_wave.h"
#include "lds_dma.h"
#include "weight_update.h"

struct GreensArgs {
    int M, na, nb, nt, nw;
    const cplx *phi, *psi;
    long psi_stride;    // 0: one trial for all walkers; M*nt: walker w uses psi + w*psi_stride
    cplx *ghalf;        // may be null (determinant only)
    cplx *gsum;         // optional [nw, na*M]: Ghalf_a + Ghalf_b (na == nb), see k_force_bias_generic
    cplx *oinv;         // optional [nw, 2, nmax, nmax]: O^-1 (O = phi^T conj(psi)), row-major, leading dim nmax
    cplx *det;          // [nw]
    cplx *det_a;        // optional [nw]: the alpha spin's determinant alone (multi-determinant trials: walkers/multi_det.py:209)
    cplx *ws;           // global workspace [nw, nmax*nmax] when O does not fit LDS
    int o_in_lds;
    int only_alive;
    const int *alive;
    int psi_real;       // every imaginary part of the (single, shared) trial is exactly zero (checked at upload)
    int skip_spin;      // with gsum: do not store the per-spin Ghalf (nobody will read it: afq_propagate_finish)
    int psi_closed;     // the alpha and beta blocks of the (single, shared) trial are bitwise equal, na == nb (checked at upload)
    unsigned long long *closed_bad;     // raised to closed_epoch by a walker whose spin blocks differ (afq_internal.h), or null
    unsigned long long closed_epoch;
    unsigned long long *counters;       // afq_counters_ext [5]: walkers that took the one-spin path
};

// One evaluation by the one-work-group kernels, between its two halves (k_small.hip): greens_fill has set the arguments and done
// the bookkeeping of the cached Green's function; launch_greens, or the fused propagator's tail, runs it.
struct GreensLaunch {
    enum Path { BIG, SMALL, LU } path;      // k_greens_big / greens_tiny_kernel, greens_small_kernel / greens_kernel
    GreensArgs a;
    WeightArgs wa;
    size_t lds;                             // SMALL: dynamic LDS of the kernel
    bool ride, inverse, wgj, tiny;
};

// Fast path for N <= 45 electrons per spin (the overlap matrix and its inverse
// fit LDS twice over).  One 512-thread workgroup per walker: waves 0-3 work on
// spin up, waves 4-7 on spin down, in lock step.
//   phase 1  O = phi_s^T conj(psi_s)            fp64 MFMA, one 16x16 tile per wave at a time
//   phase 2  in-place Gauss-Jordan inverse with row pivoting + determinant, one wave per spin,
//            the whole N x N update of a pivot step spread over the 64 lanes
//   phase 3  Ghalf_s = O^-1 phi_s^T             fp64 MFMA, A fragment from LDS
// (reference: scipy.linalg.inv + numpy.dot + slogdet, walkers/single_det.py:310-320)
#define GS_KSMAX 32       // k-steps of 4 supported by the fast Green's kernel (M <= 128)
// wa.weight != null: the hybrid / free-projection weight update of this walker (propagation/continuous.py:264-292,
// :194-200) and the driver's weight cap run right behind its determinant (a.det IS wa.ovlp_new then), which
// saves the separate weight_kernel launch of the step.
// WGJ: both spins have n <= 32 and invert by one wave each in registers (gj_wave.h); otherwise the LDS Gauss-Jordan of
// wave 0.  Two instantiations, so that neither carries the other's registers and scalars.
// The body: walker w, `smem` the work-group's dynamic LDS (launch_greens' size).  known_closed: the caller has established that
// the walker's spin blocks are bitwise equal (the propagator's resident body stores one result to both): the compare of the
// copy in LDS is left out, afq_counters_ext [5] still counts the walker and closed_bad is not touched.
// EARLY (the fused propagator's 3-multiplication tail alone; off, greens_small_kernel and the other tail compile the text they
// had): a walker whose early.on is set -- uniform over the work-group -- comes with phases 0 to 2 done by the resident body
// (k_fused_closed.h): phi_l and O^-1 of spin up lie in `smem` where this body would have left them, and the determinant of
// spin up is in early.ph / early.la of wave 7.  Such a walker is closed: afq_counters_ext [5] counts it, [8] counts the path.
struct EarlyTail {
    bool on;
    cplx ph;
    int la;
};

template <bool INVERSE, bool WGJ, bool EARLY = false>
__device__ __attribute__((always_inline)) inline void greens_small_body(const GreensArgs &a, const WeightArgs &wa, const int w,
                                                                       unsigned char *smem, const bool known_closed,
                                                                       const EarlyTail *early = nullptr) {
    __shared__ cplx ph_s[2];
    __shared__ double la_s[2];
    __shared__ unsigned long long pmax_s[2][48];
    const int tid = threadIdx.x;
    // wave-uniform on purpose (readfirstlane): the spin's electron count n and column offset derive from g, and every
    // test on them is then a scalar branch instead of an exec-mask region
    const int g = __builtin_amdgcn_readfirstlane(tid >> 8), wave = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);
    const int lane = tid & 63;
    unsigned long long *pmax = pmax_s[g];
    if ((tid & 255) < 48) pmax[tid & 255] = 0ull;
    const int M = a.M, nt = a.nt;
    const int nmax = a.na > a.nb ? a.na : a.nb;
    const int n = g == 0 ? a.na : a.nb, off = g == 0 ? 0 : a.na;
    cplx *O = (cplx *)smem + (long)g * (nmax * nmax + 2 * nmax);
    cplx *colk = O + nmax * nmax, *rowk = colk + nmax;
    int *piv = (int *)((cplx *)smem + 2L * (nmax * nmax + 2 * nmax)) + g * nmax;
    cplx *phi_l = (cplx *)smem + 2L * (nmax * nmax + 2 * nmax) + ((2 * nmax + 3) / 4 + 1);   // [M, nt] copy of the walker
    const cplx *phi_g = a.phi + (long)w * M * nt;
    const int lr = lane & 15, lk = lane >> 4;
    const int nt16 = (n + 15) >> 4;
    const int nks = (M + 3) >> 2;
    // ---- phases 0 and 1: the walker's Slater matrix into LDS, O = phi_s^T conj(psi_s) by MFMA (phi fragments from LDS, trial
    // fragments from memory).  k-steps go in groups of four.  The first sixteen trial fragments of the wave's first tile are
    // requested BEFORE the copy (they do not depend on the walker: their latency runs under phase 0), the rest right behind
    // the barrier, ahead of the first MFMA.  The MFMA loop is pipelined by hand: the four phi fragments of group g + 1 are
    // read from LDS before the twelve MFMAs of group g are issued, and there is ONE uniform branch per group -- with a branch
    // per k-step every LDS read sat in its own basic block right in front of the three MFMAs that wait for it (~800 cycles
    // per k-step measured, 64 x 3 of them MFMA).  Addresses are 32-bit offsets from wave-uniform bases.
    constexpr int NG = GS_KSMAX / 4;
    const int ng = (nks + 3) >> 2;
    // real trial (RHF / UHF orbitals of a real Hamiltonian, plane waves, lattice sites): x * y by two MFMAs per k-step
    // instead of three -- the phase is bound by the matrix pipe, two waves per SIMD.  The choice is made ONCE, around the
    // whole phase (a generic lambda instantiated for both cases): a test inside the loops is a branch per k-step.
    const bool yreal = WGJ && a.psi_real != 0;
    const char *psi_w = (const char *)(a.psi + w * a.psi_stride);
    const bool has_tile = wave < nt16 * nt16;
    bool closed = false;                                     // (set in phase01, uniform over the work-group)
    auto phase01 = [&](auto yr_tag) __attribute__((always_inline)) {
        constexpr bool YR = decltype(yr_tag)::value;
        using y_t = typename std::conditional<YR, double, cplx>::type;
        y_t yf[GS_KSMAX];
        // sixteen k-steps of trial fragments: unconditional loads of clamped rows, nothing that reads them in between (a
        // select on a loaded value in this block makes the compiler wait for every group of loads before it issues the
        // next); rows past M are zeroed where they are used
        auto load_trial = [&](int tj, const int g0) __attribute__((always_inline)) {
            const int jb = tj * 16 + lr, jbc = jb < n ? jb : n - 1;
            const unsigned col = (unsigned)(off + jbc) * 16u, rowb = (unsigned)nt * 16u;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int ks = g0 * 4 + q, p = ks * 4 + lk;
                yf[ks] = *(const y_t *)(psi_w + ((unsigned)(p < M ? p : M - 1) * rowb + col));
            }
        };
        const int tj0 = has_tile ? wave % nt16 : 0;
        if (has_tile) {
            load_trial(tj0, 0);
            if (ng > 4) load_trial(tj0, 4);
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            // the walker by LDS-DMA: 1 KB per wave and instruction straight into phi_l, all requests of a wave in flight at once
            const unsigned total = (unsigned)(M * nt) * 16u;
            const int wave8 = __builtin_amdgcn_readfirstlane(tid >> 6);
            for (unsigned b0 = (unsigned)wave8 * 1024u; b0 < total; b0 += 8 * 1024u) {
                const unsigned bo = b0 + (unsigned)lane * 16u;
                if (bo < total) glds16((const char *)phi_g + bo, (char *)phi_l + b0);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();                                         // phi_l complete
        // Closed-shell walker (round 5): the trial's spin blocks are bitwise equal (host-checked) and so are THIS walker's
        // -- an RHF run, where every operator of the step acts on both spins alike.  Checked here, on the copy in LDS, every
        // time, for this walker alone: no state, nothing to invalidate.  Then O_b = O_a, det = det_a^2, Ghalf_b = Ghalf_a
        // bit for bit, and the beta half of phases 1 - 3 is not computed (spin-sum mode only: that is the step's path).
        if (WGJ && a.psi_closed && a.gsum && !a.oinv && INVERSE) {
            if (known_closed) closed = true;
            else {
                int same = 1;
                const int na_ = a.na;
                for (int e = tid; e < M * na_; e += 512) {
                    const int p_ = e / na_, i_ = e - p_ * na_;
                    const cplx x = phi_l[p_ * nt + i_], y = phi_l[p_ * nt + na_ + i_];
                    same &= (__double_as_longlong(x.x) == __double_as_longlong(y.x)) & (__double_as_longlong(x.y) == __double_as_longlong(y.y));
                }
                closed = __syncthreads_and(same) != 0;
                if (!closed && tid == 0 && a.closed_bad) atomicMax(a.closed_bad, a.closed_epoch);
            }
            if (closed && tid == 0 && a.counters) atomicAdd(&a.counters[5], 1ull);
        }
        for (int t = wave; t < (closed && g == 1 ? 0 : nt16 * nt16); t += 4) {
            const int ti = t / nt16, tj = t % nt16;
            const int ia = ti * 16 + lr;
            const int iac = ia < n ? ia : n - 1;
            if (!WGJ && t != wave) {                             // (n <= 32: four tiles per spin, one per wave)
                load_trial(tj, 0);
                if (ng > 4) load_trial(tj, 4);
            }
            d4_t accR = {0, 0, 0, 0}, accI = {0, 0, 0, 0}, acc3 = {0, 0, 0, 0};
            cplx xa[4], xb[4];
            const unsigned xcol = (unsigned)(off + iac), xrow = (unsigned)nt;
            auto readx = [&](cplx (&x)[4], const int gq) __attribute__((always_inline)) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int p = (gq * 4 + u) * 4 + lk;
                    x[u] = phi_l[xcol + (unsigned)(p < M ? p : M - 1) * xrow];
                }
            };
            auto mf = [&](const cplx (&x)[4], const int gq) __attribute__((always_inline)) {
                const bool last = gq == ng - 1;                  // (uniform) only the last group can run past M
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool dead = last && (gq * 4 + u) * 4 + lk >= M;
                    if constexpr (YR) {
                        const double y = dead ? 0.0 : yf[gq * 4 + u];
                        accR = mfma16(x[u].x, y, accR);
                        acc3 = mfma16(x[u].y, y, acc3);
                    } else {
                        const cplx y = dead ? cmake(0.0, 0.0) : yf[gq * 4 + u];
                        // x * conj(y) by three multiplications: P1 = xr yr, P2 = xi yi, P3 = (xr + xi)(yr - yi);
                        // re = P1 + P2, im = P3 - P1 + P2 (three independent accumulator chains)
                        accR = mfma16(x[u].x, y.x, accR);
                        accI = mfma16(x[u].y, y.y, accI);
                        acc3 = mfma16(x[u].x + x[u].y, y.x - y.y, acc3);
                    }
                }
            };
            readx(xa, 0);
#pragma unroll
            for (int gq = 0; gq < NG; gq += 2) {
                if (gq < ng) {
                    if (gq + 1 < ng) readx(xb, gq + 1);
                    mf(xa, gq);
                }
                if (gq + 1 < ng) {
                    if (gq + 2 < ng) readx(xa, gq + 2 < NG ? gq + 2 : 0);
                    mf(xb, gq + 1);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = ti * 16 + lk + 4 * r, j = tj * 16 + lr;
                if (i < n && j < n) O[i * n + j] = YR ? cmake(accR[r], acc3[r]) : cmake(accR[r] + accI[r], acc3[r] - accR[r] + accI[r]);
            }
            if (WGJ) break;
        }
    };
    bool skip012 = false;                                     // (EARLY: uniform over the work-group)
    if constexpr (EARLY) skip012 = early->on;
    if (skip012) {
        closed = true;
        if (tid == 0 && a.counters) { atomicAdd(&a.counters[5], 1ull); atomicAdd(&a.counters[8], 1ull); }
        if (tid == 448) { ph_s[0] = early->ph; ph_s[1] = early->ph; la_s[0] = (double)early->la; la_s[1] = (double)early->la; }
    }
    else if (yreal) phase01(std::true_type{});
    else phase01(std::false_type{});
    if (!skip012) __syncthreads();
    // ---- phase 2
    __shared__ cplx gj_row[2][32], gj_piv[2][32];
    __shared__ int gj_prow[2][32];
    // (the two single-wave inversions run on different SIMDs: spin up on wave 0, spin down on wave 1 of its group = wave 5)
    if (WGJ) {
        if (wave == g && !(closed && g == 1) && !skip012) {
            cplx ph;
            int la;
            gj_wave32(O, n, lane, INVERSE, gj_row[g], gj_piv[g], gj_prow[g], ph, la);
            if (lane == 0) {
                ph_s[g] = ph; la_s[g] = (double)la;
                if (closed) { ph_s[1] = ph; la_s[1] = (double)la; }         // det O_b = det O_a
            }
        }
    } else if (wave == 0) {
        // det = prod of pivots, kept as (mantissa, binary exponent) so that neither log, exp nor
        // hypot sits on the per-pivot critical path
        cplx ph = cmake(1.0, 0.0);
        int la = 0;
        const int cw_shift = n <= 32 ? 5 : 6;
        const int cj = lane & ((1 << cw_shift) - 1), ri = lane >> cw_shift, rstep = 64 >> cw_shift;
        for (int k = 0; k < n; ++k) {
            // column k -> colk; pivot = first row with the largest |re|+|im| (LAPACK izamax metric):
            // one LDS atomic max on the bit pattern of the (non-negative) metric, then a ballot
            unsigned long long mbits = 0;
            if (lane < n) {
                const cplx v = O[lane * n + k];
                colk[lane] = v;
                if (lane >= k) {
                    mbits = (unsigned long long)__double_as_longlong(fabs(v.x) + fabs(v.y));
                    atomicMax(&pmax[k], mbits);
                }
            }
            __builtin_amdgcn_wave_barrier();
            const unsigned long long mx = pmax[k];
            const unsigned long long hit = __ballot(lane >= k && lane < n && mbits == mx);
            const int p = hit ? __ffsll((long long)hit) - 1 : k;
            if (p != k) {
                for (int j = lane; j < n; j += 64) {
                    const cplx t = O[k * n + j];
                    O[k * n + j] = O[p * n + j];
                    O[p * n + j] = t;
                }
                if (lane == 0) { const cplx t = colk[k]; colk[k] = colk[p]; colk[p] = t; }
            }
            if (lane == 0) piv[k] = p;
            __builtin_amdgcn_wave_barrier();
            const cplx d = colk[k];
            ph = cmul(ph, p != k ? cmake(-d.x, -d.y) : d);
            {
                int e;
                (void)frexp(fmax(fabs(ph.x), fabs(ph.y)), &e);
                ph = cmake(ldexp(ph.x, -e), ldexp(ph.y, -e));
                la += e;
            }
            const double dn = 1.0 / (d.x * d.x + d.y * d.y);
            const cplx dinv = cmake(d.x * dn, -d.y * dn);
            for (int j = lane; j < n; j += 64) rowk[j] = cmul(O[k * n + j], dinv);
            __builtin_amdgcn_wave_barrier();
            if (n <= 32) {
                // n x n update with every LDS read of the step in flight before the arithmetic:
                // lane (ri, cj) owns rows ri, ri+2, ... of column cj; 16 rows per lane, unrolled
                if (cj < n && (INVERSE || cj > k)) {
                    const cplx rk = rowk[cj];
                    cplx v[16], f[16];
#pragma unroll
                    for (int t = 0; t < 16; ++t) {
                        const int i = ri + 2 * t;
                        if (i < n) { v[t] = O[i * n + cj]; f[t] = colk[i]; }
                    }
#pragma unroll
                    for (int t = 0; t < 16; ++t) {
                        const int i = ri + 2 * t;
                        if (i < n && (INVERSE || i > k)) {
                            cplx o;
                            if (INVERSE && i == k) o = (cj == k) ? dinv : rk;
                            else if (INVERSE && cj == k) { const cplx m = cmul(f[t], dinv); o = cmake(-m.x, -m.y); }
                            else {
                                o = v[t];
                                o.x = fma(-f[t].x, rk.x, o.x); o.x = fma(f[t].y, rk.y, o.x);
                                o.y = fma(-f[t].x, rk.y, o.y); o.y = fma(-f[t].y, rk.x, o.y);
                            }
                            O[i * n + cj] = o;
                        }
                    }
                }
            } else if (INVERSE) {
                if (cj < n) {
                    const cplx rk = rowk[cj];
                    for (int i = ri; i < n; i += rstep) {
                        cplx v;
                        if (i == k) v = (cj == k) ? dinv : rk;
                        else {
                            const cplx f = colk[i];
                            if (cj == k) { const cplx t = cmul(f, dinv); v = cmake(-t.x, -t.y); }
                            else {
                                v = O[i * n + cj];
                                v.x = fma(-f.x, rk.x, v.x); v.x = fma(f.y, rk.y, v.x);
                                v.y = fma(-f.x, rk.y, v.y); v.y = fma(-f.y, rk.x, v.y);
                            }
                        }
                        O[i * n + cj] = v;
                    }
                }
            } else {
                if (cj < n && cj > k) {
                    const cplx rk = rowk[cj];
                    for (int i = k + 1 + ri; i < n; i += rstep) {
                        const cplx f = colk[i];
                        cplx v = O[i * n + cj];
                        v.x = fma(-f.x, rk.x, v.x); v.x = fma(f.y, rk.y, v.x);
                        v.y = fma(-f.x, rk.y, v.y); v.y = fma(-f.y, rk.x, v.y);
                        O[i * n + cj] = v;
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (INVERSE) {
            for (int k = n - 1; k >= 0; --k) {
                const int p = piv[k];
                if (p != k) {
                    for (int i = lane; i < n; i += 64) {
                        const cplx t = O[i * n + k];
                        O[i * n + k] = O[i * n + p];
                        O[i * n + p] = t;
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (lane == 0) { ph_s[g] = ph; la_s[g] = (double)la; }
    }
    __syncthreads();
    // (the last wave: its phase-3 item is the half-width one, the first wave's is full)
    if (tid == 448) {
        const cplx p2 = cmul(ph_s[0], ph_s[1]);
        const int e = (int)(la_s[0] + la_s[1]);
        a.det[w] = cmake(ldexp(p2.x, e), ldexp(p2.y, e));
        if (a.det_a) a.det_a[w] = cmake(ldexp(ph_s[0].x, (int)la_s[0]), ldexp(ph_s[0].y, (int)la_s[0]));
        if (wa.weight) weight_update_and_cap(wa, w);
    }
    if (INVERSE && a.oinv) {
        cplx *oo = a.oinv + ((long)w * 2 + g) * nmax * nmax;
        for (int e = tid & 255; e < n * n; e += 256) oo[(e / n) * nmax + (e % n)] = O[e];
    }
    // ---- phase 3: Ghalf = O^-1 phi^T.  Work item = (row tile of O^-1, PAIR of column tiles): the O^-1 fragments of the
    // row tile are read from LDS once per item and kept in registers, the two column tiles give six independent
    // accumulators (3-multiplication complex product: P1 = xr yr, P2 = xi yi, P3 = (xr + xi)(yr + yi)), and every LDS
    // read is unconditional (clamped index, zero by select) -- the previous loop re-read O^-1 for every column tile,
    // ran four dependent MFMAs per contraction step on two accumulators and branched around its operand reads.
    // With a.gsum (na == nb, host-checked) every wave of the work-group takes items of BOTH spins, so that the two Green's
    // functions of an element meet in one lane and their sum (what the force bias contracts when both spins share the
    // Cholesky block) is stored along.
    if (INVERSE && a.ghalf) {
        const bool both = a.gsum != nullptr;
        const int mt16 = (M + 15) >> 4, npair = (mt16 + 1) >> 1;
        const int first = both ? __builtin_amdgcn_readfirstlane(tid >> 6) : wave, stride = both ? 8 : 4;
        const int s_lo = both ? 0 : g, s_hi = both ? 2 : g + 1;
        const int nn = both ? a.na : n, nt16x = (nn + 15) >> 4;
        for (int it = first; nn > 0 && it < nt16x * npair; it += stride) {
            const int ti = it % nt16x, tc0 = 2 * (it / nt16x), tc1 = tc0 + 1;
            const bool two = tc1 < mt16;
            const int c0 = tc0 * 16 + lr, c1 = tc1 * 16 + lr;
            const int c0c = c0 < M ? c0 : M - 1, c1c = c1 < M ? c1 : M - 1;
            d4_t sra = {0, 0, 0, 0}, sia = {0, 0, 0, 0}, srb = {0, 0, 0, 0}, sib = {0, 0, 0, 0};
            for (int s = s_lo; s < (closed ? 1 : s_hi); ++s) {
                const int ns = s ? a.nb : a.na, offs = s ? a.na : 0;
                const cplx *Os = (const cplx *)smem + (long)s * (nmax * nmax + 2 * nmax);
                cplx *gh = a.ghalf + ((long)w * nt + offs) * M;
                const int nks3 = (ns + 3) >> 2;                      // ns <= 45: nks3 <= 12
                const int ia = ti * 16 + lr, iac = ia < ns ? ia : ns - 1;
                cplx xf[12];
#pragma unroll
                for (int ks = 0; ks < 12; ++ks) {
                    const int j = ks * 4 + lk, jc = j < ns ? j : ns - 1;
                    const cplx x = Os[iac * ns + jc];
                    xf[ks] = (ks < nks3 && j < ns && ia < ns) ? x : cmake(0.0, 0.0);
                }
                d4_t p1a = {0, 0, 0, 0}, p2a = {0, 0, 0, 0}, p3a = {0, 0, 0, 0};
                d4_t p1b = {0, 0, 0, 0}, p2b = {0, 0, 0, 0}, p3b = {0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < 12; ++ks) {
                    if (ks < nks3) {
                        const int j = ks * 4 + lk, jc = j < ns ? j : ns - 1;
                        // (xf is zero wherever the contraction index runs past ns; columns past M are never stored)
                        const cplx y0 = phi_l[c0c * nt + offs + jc], y1 = phi_l[c1c * nt + offs + jc];
                        const cplx x = xf[ks];
                        const double xs = x.x + x.y;
                        p1a = mfma16(x.x, y0.x, p1a);
                        p2a = mfma16(x.y, y0.y, p2a);
                        p3a = mfma16(xs, y0.x + y0.y, p3a);
                        if (two) {
                            p1b = mfma16(x.x, y1.x, p1b);
                            p2b = mfma16(x.y, y1.y, p2b);
                            p3b = mfma16(xs, y1.x + y1.y, p3b);
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = ti * 16 + lk + 4 * r;
                    const double ra = p1a[r] - p2a[r], ima = p3a[r] - p1a[r] - p2a[r];
                    const double rb = p1b[r] - p2b[r], imb = p3b[r] - p1b[r] - p2b[r];
                    if (i < ns && c0 < M && !a.skip_spin) gh[(long)i * M + c0] = cmake(ra, ima);
                    if (two && i < ns && c1 < M && !a.skip_spin) gh[(long)i * M + c1] = cmake(rb, imb);
                    sra[r] += ra; sia[r] += ima; srb[r] += rb; sib[r] += imb;
                    if (closed) {
                        // Ghalf_b = Ghalf_a: the same values into the beta rows, and twice into the spin sum (x + x: exact)
                        cplx *ghb = gh + (long)a.na * M;
                        if (i < ns && c0 < M && !a.skip_spin) ghb[(long)i * M + c0] = cmake(ra, ima);
                        if (two && i < ns && c1 < M && !a.skip_spin) ghb[(long)i * M + c1] = cmake(rb, imb);
                        sra[r] += ra; sia[r] += ima; srb[r] += rb; sib[r] += imb;
                    }
                }
            }
            if (both) {
                cplx *gs = a.gsum + (long)w * a.na * M;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = ti * 16 + lk + 4 * r;
                    if (i < a.na && c0 < M) gs[(long)i * M + c0] = cmake(sra[r], sia[r]);
                    if (two && i < a.na && c1 < M) gs[(long)i * M + c1] = cmake(srb[r], sib[r]);
                }
            }
        }
    }
}
