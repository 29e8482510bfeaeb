// Closed-shell body of the fused propagator with the walker's HS potential V resident in registers
// (included by k_fused.hip behind PropFusedArgs; entered from prop_fused_kernel<false, 7> for a walker it has found closed).
//
//   phi <- B . [ sum_{n<=order} V^n / n! ] . B . phi      on the alpha half; the result is stored to both spin blocks
//
// Shape class (host-checked, see k_prop_closed_resident): one real one-body matrix for both spins, na == nb in 17 .. 32,
// M in 97 .. 104, order > 0.  KS = ceil(M / 4) k-steps of one v_mfma_f64_16x16x4 (25 or 26): the k loop of every product is
// fully unrolled over KS so that each A fragment of V has a register of its own.
//   * wave r (0 .. 6) owns row tile r and both alpha column slots.  Its A fragments of V -- lane (lr, lk) holds
//     V[16 r + lr][4 s + lk] for k-step s, one 16-byte global load each -- are loaded ONCE per walker and step, under the
//     opening one-body pass, and serve all `order` Taylor products: no operand ring, no chunk barrier, no DMA.
//     Wave 7 takes part in the fill of T and in the barriers -- and, MUL3, multiplies the upper k-steps of slot 1 of row tiles
//     4-6 in every Taylor product (the split deal: see the products) -- and, EARLY (the 3-multiplication tail kernel with psi^H B
//     at hand, afq_set_step_tail_overlap), stages psi^H B in LDS and inverts the tail's overlap matrix under the closing pass:
//     see the end of the body.
//   * T (the right-hand operand, alpha half: M x 32 complex) lives in LDS in B-fragment order [k-step][slot][64 lanes x 16 B]
//     (lane (lr, lk) of k-step s, slot j: T[4 s + lk][16 j + lr]), 2 KB per k-step, KS * 2 KB <= 52 KB per image.  Two
//     images: a product reads one and writes the other, so a hand-over is ONE barrier.  The accumulator of row tile r
//     (register q, lane (lr, lk) = row 16 r + 4 q + lk) is exactly the lane image of k-step 4 r + q: the write-back is a
//     lane-linear ds_write_b128.  Both images lie below the operand ring of the streamed body (2 * KS * 2 KB <= NCH * 8 KB).
//   * the one-body passes stream the real parts of BH1 (8 bytes per lane and k-step, L2 resident, shared by all walkers)
//     into registers ahead of their k loop: two real products per slot.
//   * the Taylor products are plain 4-multiplication complex products (MUL3, launches with the Green's function tail: the
//     3-multiplication form of taylor(), im = P3 - P1 - P2) (re = P1 - P2 at the end, im accumulated in one
//     register set): k ascending in steps of 4, T_n = product / n, sum += T_n as in taylor().  Four MFMAs per k-step and slot
//     where taylor()'s 3-multiplication form has three: see DESIGN section 4 for why this body pays them.  MUL3 deals the
//     products over all four SIMDs: slot 1 of row tiles 4-6 is a k sum in two pieces, the owner's and wave 7's.
//   * EARLY with the step hand-over (StepHandoverArgs, afq_set_step_handover): under wave 7's inversion the other waves also
//     make the opening pass of the NEXT step, (B B) S, and store it as an image of T in memory; a walker that finds one from the
//     launch before starts at the Taylor products.  See "Hand-over" in the body.
// Rows and k >= M read a zero page: the padding of T stays zero through every product.
#pragma once

#define PCR_LDS(p) ((__attribute__((address_space(3))) unsigned char *)(p))

template <int KS, bool MUL3, bool EARLY = false>
__device__ __attribute__((always_inline)) inline void prop_closed_resident(const PropFusedArgs &a, unsigned char *smem_,
                                                                           cplx *phi, const cplx *vhs,
                                                                           const double *psiB = nullptr, EarlyTail *et = nullptr,
                                                                           const StepHandoverArgs *ho = nullptr, const bool handed_ = false) {
    auto *smem = PCR_LDS(smem_);
    // EARLY alone: the walker starts from the image of T_0 the launch before left in ho->t0_next (see "Hand-over" below)
    const bool handed = EARLY && handed_;                       // work-group uniform
    typedef __attribute__((address_space(3))) d2_t lds_d2;
    typedef __attribute__((address_space(3))) double lds_f64;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = a.M, nt = a.nt, na = a.na;
    constexpr unsigned TB = KS * 2048;                          // one image of T
    const bool mul = wave < 7;                                  // wave-uniform
    // MUL3: the split deal of the Taylor products (see the products below).  Slot 1 of row tiles 4-6 is cut along k at k-step
    // KH: the owner multiplies [0, KH), wave 7 the KU k-steps [KH, KS) of all three.
    constexpr int KH = (KS + 1) / 2, KU = KS - KH;
    constexpr unsigned PB = 2 * TB;                             // psi^H B as A fragments (EARLY), KS * 1 KB
    constexpr unsigned PP = PB + KS * 1024;                     // wave 7's partial products: 3 units x 64 lanes x 64 B
    static_assert(PP + 3 * 4096 <= 13 * 8192 + PF_D * 16384, "the partial products lie inside the launch's LDS (M > 96)");
    // The lane's coordinates are derived afresh from the thread index wherever a stage needs them (laundered through an
    // empty asm): addresses and indices of a later stage then hold no registers across the unrolled products.
    auto lane_id = [&]() __attribute__((always_inline)) -> int {
        int t = tid;
        asm volatile("" : "+v"(t));
        return t & 63;
    };

    // ---- phi[w], alpha half -> image 0 (B-fragment order), padding zeroed
    // (EARLY with an odd `order`: image 1, so that the Taylor sum ends in image 1 for either parity and image 0, where the
    //  tail's overlap matrix lies, is dead behind the last product)
    const unsigned base0 = (EARLY && (a.order & 1)) ? TB : 0u;
    // Hand-over (EARLY, afq_set_step_handover): T_0 = B phi of THIS step was made by the launch before, as (B B) S under its
    // inversion, and lies in ho->t0_next[w] as the image itself -- same linear offsets, padding included.  The walker then
    // reads no phi at all: the work-group requests the image (16 bytes per thread and trip) and, right behind it, waves 0-6
    // their own accumulator slice of it (the first term of the sum) and their fragments of V; the image goes to LDS ahead of
    // the barrier in front of the Taylor products, V stays in flight as on the other path.
    constexpr int NCP = (KS * 128 + PF_NT - 1) / PF_NT;
    d2_t cp[NCP];
    if (handed) {
        const d2_t *t0 = (const d2_t *)(ho->t0_next + (size_t)blockIdx.x * TB);
#pragma unroll
        for (int i = 0; i < NCP; ++i) {
            const int e = tid + i * PF_NT;
            cp[i] = t0[e < KS * 128 ? e : 0];
        }
    } else {
        for (int e = tid; e < KS * 128; e += PF_NT) {
            const int k = 4 * (e >> 7) + ((e >> 4) & 3), col = 16 * ((e >> 6) & 1) + (e & 15);
            const bool ok = k < M && col < na;
            const cplx v = phi[ok ? k * nt + col : 0];
            ((lds_d2 *)(smem + base0))[e] = ok ? (d2_t){v.x, v.y} : (d2_t){0.0, 0.0};
        }
        __syncthreads();
    }

    // A fragments of Re(BH1), this wave's row tile
    auto load_b = [&](double (&bh)[KS]) __attribute__((always_inline)) {
        const int lane = lane_id(), lk = lane >> 4, row = wave * 16 + (lane & 15);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int k = 4 * s + lk;
            const double *p = (row < M && k < M) ? &a.BH1[row * M + k].x : (const double *)a.zero16;
            bh[s] = *p;
        }
    };
    // one-body product of image `src`: P1 + i P2 = Re(BH1)[row tile] . T
    auto one_body = [&](const unsigned src, const double (&bh)[KS], d4_t (&P1)[2], d4_t (&P2)[2]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 2; ++j) { P1[j] = (d4_t){0, 0, 0, 0}; P2[j] = (d4_t){0, 0, 0, 0}; }
        const auto *tb = smem + src + lane_id() * 16;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const d2_t b = *(const lds_d2 *)(tb + (s * 2 + j) * 1024);
                P1[j] = mfma16(bh[s], b[0], P1[j]);
                P2[j] = mfma16(bh[s], b[1], P2[j]);
            }
        }
    };
    // accumulator layout -> image `dst`: register q of row tile `wave` is k-step 4 wave + q (k-steps past KS do not exist)
    auto put = [&](const unsigned dst, const d4_t (&re)[2], const d4_t (&im)[2]) __attribute__((always_inline)) {
        auto *tb = smem + dst + lane_id() * 16;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (4 * wave + q < KS) {
#pragma unroll
                for (int j = 0; j < 2; ++j) *(lds_d2 *)(tb + ((4 * wave + q) * 2 + j) * 1024) = (d2_t){re[j][q], im[j][q]};
            }
    };

    // ---- The opening of a wave that multiplies (0 .. 6): its fragments of V (av: resident for the whole step) and the first
    // term of the running Taylor sum (SR, SI).  A lambda, as the two stages below: MUL3 instantiates the opening and the products
    // once for each class of waves of its deal, each with registers of its own (see the products).
    auto open_owner = [&](d2_t (&av)[KS], d4_t (&SR)[2], d4_t (&SI)[2]) __attribute__((always_inline)) {
        // ---- V fragments: issued behind the operands of the opening pass (or behind the handed first term), and consumed from
        // the first Taylor product on -- the loads travel under that pass
        auto load_v = [&]() __attribute__((always_inline)) {
            const int lane = lane_id(), lk = lane >> 4, row = wave * 16 + (lane & 15);   // this lane's row and k of the A operands
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const int k = 4 * s + lk;
                // upper-triangle storage of V: element (row, k < row) lives at (k, row)
                const int off = (a.vhs_upper && k < row) ? k * M + row : row * M + k;
                const d2_t *p = (row < M && k < M) ? (const d2_t *)(vhs + off) : (const d2_t *)a.zero16;
                av[s] = *p;
            }
        };
        // (either path whole, so that the operands of the opening pass and the handed image never hold registers together)
        if (handed) {
            // register q of row tile `wave`, slot j = lane image of k-step 4 wave + q, slot j (see put)
            const d2_t *t0 = (const d2_t *)(ho->t0_next + (size_t)blockIdx.x * TB) + lane_id();
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const d2_t v = 4 * wave + q < KS ? t0[((4 * wave + q) * 2 + j) * 64] : (d2_t){0.0, 0.0};
                    SR[j][q] = v[0]; SI[j][q] = v[1];
                }
            load_v();
        } else {
            double bh[KS];
            load_b(bh);
            load_v();
            // ---- T_0 = B phi: image 0 -> image 1, and the first term of the sum
            one_body(base0, bh, SR, SI);
            put(base0 ^ TB, SR, SI);
        }
    };
    // EARLY: wave 7, idle here, stages psi^H B in the free LDS above both images as A fragments -- [row tile t of 16 trial
    // orbitals][k-step s][64 lanes x 8 B], lane (lr, lk) = psiB[16 t + lr][4 s + lk], 2 * KS * 512 B <= 26 KB of the 48 KB --
    // under the opening pass; every wave reads its share behind the last Taylor product (any barrier in between publishes it)
    auto stage_psib = [&]() __attribute__((always_inline)) {
        const int lane = lane_id(), lk = lane >> 4, lr = lane & 15;
        double pv[2][KS];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const int j = 16 * t + lr, k = 4 * s + lk;
                const double *p = (j < na && k < M) ? psiB + j * M + k : (const double *)a.zero16;
                pv[t][s] = *p;
            }
        auto *pb = smem + PB + lane * 8;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int s = 0; s < KS; ++s) *(lds_f64 *)(pb + (t * KS + s) * 512) = pv[t][s];
    };
    // the handed image of T_0, requested above, goes to LDS: every thread, ahead of the barrier in front of the products
    auto copy_t0 = [&]() __attribute__((always_inline)) {
        if (handed) {
#pragma unroll
            for (int i = 0; i < NCP; ++i) {
                const int e = tid + i * PF_NT;
                if (e < KS * 128) ((lds_d2 *)(smem + (base0 ^ TB)))[e] = cp[i];
            }
        }
    };
    // ---- Taylor products from the resident fragments: image cur -> image cur ^ TB, one barrier each
    unsigned cur = base0 ^ TB;
    if constexpr (!MUL3) {
    // (the statements of open_owner without the hand-over, which is MUL3's alone)
    static_assert(MUL3 || !EARLY, "the early tail and the hand-over belong to the 3-multiplication tail kernel");
    d2_t av[KS];                                                // V, this wave's row tile: resident for the whole step
    d4_t SR[2], SI[2];                                          // running Taylor sum
    if (mul) {
        double bh[KS];
        load_b(bh);
        const int lane = lane_id(), lk = lane >> 4, row = wave * 16 + (lane & 15);   // this lane's row and k of the A operands
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int k = 4 * s + lk;
            const int off = (a.vhs_upper && k < row) ? k * M + row : row * M + k;
            const d2_t *p = (row < M && k < M) ? (const d2_t *)(vhs + off) : (const d2_t *)a.zero16;
            av[s] = *p;
        }
        one_body(base0, bh, SR, SI);
        put(base0 ^ TB, SR, SI);
    }
    lds_barrier();
    for (int n = 1; n <= a.order; ++n) {
        if (mul) {
            double inv_n = 1.0 / n;
            asm volatile("" : "+v"(inv_n));
            d4_t P1[2], P2[2], P3[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) { P1[j] = (d4_t){0, 0, 0, 0}; P2[j] = (d4_t){0, 0, 0, 0}; P3[j] = (d4_t){0, 0, 0, 0}; }
            const auto *tb = smem + cur + lane_id() * 16;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                // (laundered at the k-step itself, so that the first product waits for the loads of V one fragment at a time)
                asm volatile("" : "+v"(av[s]));
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    // (both halves of the imaginary part go into one accumulator, two independent MFMAs apart)
                    const d2_t b = *(const lds_d2 *)(tb + (s * 2 + j) * 1024);
                    P3[j] = mfma16(av[s][0], b[1], P3[j]);
                    P1[j] = mfma16(av[s][0], b[0], P1[j]);
                    P2[j] = mfma16(av[s][1], b[1], P2[j]);
                    P3[j] = mfma16(av[s][1], b[0], P3[j]);
                }
            }
            // T_n = product / n is the next right-hand operand; after the last term the image receives the SUM instead
            d4_t re[2], im[2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    re[j][q] = (P1[j][q] - P2[j][q]) * inv_n;
                    im[j][q] = P3[j][q] * inv_n;
                    SR[j][q] += re[j][q]; SI[j][q] += im[j][q];
                }
            if (n == a.order) put(cur ^ TB, SR, SI);
            else put(cur ^ TB, re, im);
        }
        lds_barrier();
        cur ^= TB;
    }
    } else {
    // MUL3, the split deal: taylor()'s form, P1 = ar br, P2 = ai bi, P3 = (ar + ai)(br + bi) (the sums are made per k-step, so
    // that no fragment of V needs a third resident register), three MFMAs per unit (row tile, slot) and k-step, 14 units.
    // Waves r and r + 4 share SIMD r, so the plain deal (wave r: both slots of row tile r) loads SIMDs 0-2 with 4 units and
    // SIMD 3 with 2.  Dealt here, in units of 3 KS MFMAs:
    //   waves 0-3   both slots of their row tile, every k-step                                   2
    //   waves 4-6   slot 0 of their row tile, every k-step; slot 1 over the k-steps [0, KH)      1 + KH / KS
    //   wave 7      slot 1 of row tiles 4, 5, 6 over the k-steps [KH, KS), one after the other   3 KU / KS
    // -- at KS = 25: 264 MFMAs on SIMDs 0-2 and 258 on SIMD 3, where the plain deal has 300 and 150.  Not one MFMA more or
    // fewer is issued.  Wave 7 writes each unit's partial (P1 - P2, P3 - P1 - P2), lane-linearly as it holds it, into the LDS
    // above psi^H B; one more barrier per product; the owner then adds it to its own -- own (lower k) + wave 7's (upper k), in
    // that order on every path -- ahead of the division by n.
    // The three classes of waves run the loop over `order` in a copy each, in the arms of a wave-uniform branch: a single loop
    // would hold the owners' fragments and wave 7's in registers side by side, and the kernel has one register budget for
    // all eight waves.  Every copy crosses the same two barriers per product, `order` times, and nothing else waits.
    auto kstep = [&](const d2_t &v, const unsigned char __attribute__((address_space(3))) *b_, d4_t &p1, d4_t &p2, d4_t &p3)
        __attribute__((always_inline)) {
        const d2_t b = *(const lds_d2 *)b_;
        p1 = mfma16(v[0], b[0], p1);
        p2 = mfma16(v[1], b[1], p2);
        p3 = mfma16(v[0] + v[1], b[0] + b[1], p3);
    };
    // One copy of the loop over `order` for the owners of whole units (WHOLE: waves 0-3) and one for the owners of split ones
    // (waves 4-6), each a straight run of MFMAs.
    auto owners = [&](auto whole_) __attribute__((always_inline)) {
        constexpr bool WHOLE = decltype(whole_)::value;
        d2_t av[KS];
        d4_t SR[2], SI[2];
        open_owner(av, SR, SI);
        copy_t0();
        lds_barrier();
        for (int n = 1; n <= a.order; ++n) {
            double inv_n = 1.0 / n;
            asm volatile("" : "+v"(inv_n));
            d4_t P1[2], P2[2], P3[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) { P1[j] = (d4_t){0, 0, 0, 0}; P2[j] = (d4_t){0, 0, 0, 0}; P3[j] = (d4_t){0, 0, 0, 0}; }
            const auto *tb = smem + cur + lane_id() * 16;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                // (laundered at the k-step itself, so that the first product waits for the loads of V one fragment at a time)
                asm volatile("" : "+v"(av[s]));
#pragma unroll
                for (int j = 0; j < ((WHOLE || s < KH) ? 2 : 1); ++j) kstep(av[s], tb + (s * 2 + j) * 1024, P1[j], P2[j], P3[j]);
                // (the split run is scheduled in stretches of four k-steps: left to itself the scheduler requests operands
                //  and adds a dozen k-steps ahead, and the run no longer fits the registers)
                if (!WHOLE && (s & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
            d4_t re[2], im[2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    re[j][q] = P1[j][q] - P2[j][q];
                    im[j][q] = P3[j][q] - P1[j][q] - P2[j][q];
                }
            // T_n = product / n is the next right-hand operand; after the last term the image receives the SUM instead
            auto finish = [&]() __attribute__((always_inline)) {
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        re[j][q] *= inv_n;
                        im[j][q] *= inv_n;
                        SR[j][q] += re[j][q]; SI[j][q] += im[j][q];
                    }
                if (n == a.order) put(cur ^ TB, SR, SI);
                else put(cur ^ TB, re, im);
            };
            if constexpr (WHOLE) finish();
            lds_barrier();                                          // wave 7's partials are the work-group's
            if constexpr (!WHOLE) {
                const auto *pp = smem + PP + (wave - 4) * 4096 + lane_id() * 16;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const d2_t u = *(const lds_d2 *)(pp + q * 1024);
                    re[1][q] += u[0];
                    im[1][q] += u[1];
                }
                finish();
            }
            lds_barrier();
            cur ^= TB;
        }
    };
    if (wave < 4) {
        owners(std::true_type());
    } else if (mul) {
        owners(std::false_type());
    } else {
        // wave 7: its A fragments of V -- rows 64 .. 111, k-steps KH .. KS - 1, addressed as the owners address theirs -- are
        // requested once, behind the staging of psi^H B (whose registers are dead by now) and ahead of the barrier
        if constexpr (EARLY) stage_psib();
        copy_t0();
        d2_t av7[3][KU];
        asm volatile("" ::: "memory");
        {
            const int lane = lane_id(), lk = lane >> 4;
#pragma unroll
            for (int u = 0; u < 3; ++u)
#pragma unroll
                for (int i = 0; i < KU; ++i) {
                    const int row = (4 + u) * 16 + (lane & 15), k = 4 * (KH + i) + lk;
                    const int off = (a.vhs_upper && k < row) ? k * M + row : row * M + k;
                    const d2_t *p = (row < M && k < M) ? (const d2_t *)(vhs + off) : (const d2_t *)a.zero16;
                    av7[u][i] = *p;
                }
        }
        lds_barrier();
        for (int n = 1; n <= a.order; ++n) {
            const auto *tb = smem + cur + 1024 + lane_id() * 16;
            auto *pp = smem + PP + lane_id() * 16;
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                d4_t Q1 = {0, 0, 0, 0}, Q2 = {0, 0, 0, 0}, Q3 = {0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < KU; ++i) {
                    asm volatile("" : "+v"(av7[u][i]));
                    kstep(av7[u][i], tb + (KH + i) * 2048, Q1, Q2, Q3);
                    if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);    // (as in the owners' split run)
                }
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *(lds_d2 *)(pp + u * 4096 + q * 1024) = (d2_t){Q1[q] - Q2[q], Q3[q] - Q1[q] - Q2[q]};
                __builtin_amdgcn_sched_barrier(0);
            }
            lds_barrier();
            lds_barrier();
            cur ^= TB;
        }
    }
    }

    if constexpr (EARLY) {
        // ---- The tail's overlap matrix first, its inverse under the closing pass.
        // phi' = B S with S the Taylor sum in image 1 (= cur), so O = phi'^T conj(psi) = (psiB S)^T with psiB = psi^H B (real,
        // made on the host once per upload, staged in LDS above).  LDS from here on:
        //   [0, TB)         image 0, dead: the tail's carve of O (offset 0, where wave 7 inverts it in place) and, in spin down's
        //                   block behind it -- which a closed walker's tail never touches -- the scratch of gj_wave32
        //   [TB, 2 TB)      image 1 = S, read by the overlap units and by the closing pass
        //   [2 TB, + 26 KB) psiB as A fragments
        //   the tail's copy of the walker (phi_l) overlaps all three: written behind the last barrier below
        // 1. the eight waves multiply the 2 x 2 tiles x (Re, Im) of psiB . S, one unit of KS MFMAs each (wave = 4 t + 2 j + part:
        //    row tile t of psiB, column slot j of S), and store their halves of O's entries;
        // 2. barrier: O is complete;
        // 3. wave 7 inverts O (gj_wave32, ~33 k cycles) WHILE waves 0-6 run the closing one-body pass from S and store phi' to
        //    both spin blocks of the walker, keeping their accumulators;
        // 4. barrier: S is dead, O^-1 lies where the tail reads it;
        // 5. waves 0-6 write their accumulators into phi_l; the barrier in front of the tail (prop_fused_kernel) publishes them.
        // Every wave crosses every barrier, none waits for another anywhere else.
        const int nn = na, nsq = nn * nn + 2 * nn;                  // the tail's carve (greens_small_body, nmax = na = nb)
        cplx *O = (cplx *)smem_;
        cplx *phi_l = (cplx *)smem_ + 2L * nsq + ((2 * nn + 3) / 4 + 1);
        {
            const int t = wave >> 2, j = (wave >> 1) & 1, part = wave & 1;     // wave-uniform
            const auto *pa = smem + PB + t * (KS * 512) + lane_id() * 8;
            const auto *tb = smem + cur + j * 1024 + part * 8 + lane_id() * 16;
            d4_t acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};               // even and odd k-steps: two chains per wave
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const double x = *(const lds_f64 *)(pa + s * 512), y = *(const lds_f64 *)(tb + s * 2048);
                if (s & 1) acc1 = mfma16(x, y, acc1);
                else acc0 = mfma16(x, y, acc0);
            }
            // register q, lane (lr, lk): (psiB S)[16 t + 4 q + lk][16 j + lr] = O[16 j + lr][16 t + 4 q + lk]
            const int lane = lane_id(), lr = lane & 15, lk = lane >> 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = 16 * j + lr, jj = 16 * t + 4 * q + lk;
                if (i < nn && jj < nn) ((double *)&O[i * nn + jj])[part] = acc0[q] + acc1[q];
            }
        }
        lds_barrier();
        d4_t P1[2], P2[2];
        if (mul) {
            double bh[KS];
            load_b(bh);
            one_body(cur, bh, P1, P2);
            const int lane = lane_id(), lr = lane & 15, lk = lane >> 4;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int orow = wave * 16 + lk + 4 * q, col = 16 * j + lr;
                    if (orow < M && col < na) {
                        const cplx v = cmake(P1[j][q], P2[j][q]);
                        phi[(long)orow * nt + col] = v;
                        phi[(long)orow * nt + na + col] = v;
                    }
                }
            // Hand-over, producing side: the opening pass of the NEXT step, T_0 = B phi' = (B B) S, from the same image with
            // the A fragments of B2 = B B (host-made, as psiB), still under wave 7's inversion; its accumulators are stored
            // lane-linearly as the image the consumer copies (put's layout: all KS k-steps x 2 slots, padding included).
            // Deal: wave 3 shares SIMD 3 with the inverting wave 7, and fp64 MFMAs beside the inversion lengthen it.  A result
            // that is only stored needs no fixed owner, so wave 3 sits this pass out and the two units of its row tile go to
            // waves 4 and 5 (SIMDs 0 and 1: three units each, slot wave - 4 of row tile 3 as the third).
            if (ho->produce && wave != 3) {
                const bool third = wave == 4 || wave == 5;          // wave-uniform
                auto load_b2 = [&](const int rt, double (&bf)[KS]) __attribute__((always_inline)) {
                    const int ln = lane_id(), hk = ln >> 4, hrow = rt * 16 + (ln & 15);
#pragma unroll
                    for (int s = 0; s < KS; ++s) {
                        const int k = 4 * s + hk;
                        const double *p = (hrow < M && k < M) ? ho->B2 + hrow * M + k : (const double *)a.zero16;
                        bf[s] = *p;
                    }
                };
                auto store_t0 = [&](const int rt, const int j, const d4_t &re, const d4_t &im) __attribute__((always_inline)) {
                    d2_t *t0 = (d2_t *)(ho->t0_next + (size_t)blockIdx.x * TB) + lane_id();
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (4 * rt + q < KS) t0[((4 * rt + q) * 2 + j) * 64] = (d2_t){re[q], im[q]};
                };
                d4_t Q1[2], Q2[2];
                load_b2(wave, bh);
                if (third) {
                    double b3[KS];
                    load_b2(3, b3);
                    const int j3 = wave - 4;
                    d4_t X1 = {0, 0, 0, 0}, X2 = {0, 0, 0, 0};
#pragma unroll
                    for (int j = 0; j < 2; ++j) { Q1[j] = (d4_t){0, 0, 0, 0}; Q2[j] = (d4_t){0, 0, 0, 0}; }
                    const auto *tb = smem + cur + lane_id() * 16;
                    const auto *tx = tb + j3 * 1024;
#pragma unroll
                    for (int s = 0; s < KS; ++s) {
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const d2_t b = *(const lds_d2 *)(tb + (s * 2 + j) * 1024);
                            Q1[j] = mfma16(bh[s], b[0], Q1[j]);
                            Q2[j] = mfma16(bh[s], b[1], Q2[j]);
                        }
                        const d2_t b = *(const lds_d2 *)(tx + s * 2048);
                        X1 = mfma16(b3[s], b[0], X1);
                        X2 = mfma16(b3[s], b[1], X2);
                    }
                    store_t0(3, j3, X1, X2);
                } else {
                    one_body(cur, bh, Q1, Q2);
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) store_t0(wave, j, Q1[j], Q2[j]);
            }
        } else {
            cplx *scr = O + nsq;                                    // spin down's block: 32 + 32 complex, 32 ints
            gj_wave32(O, nn, lane_id(), true, scr, scr + 32, (int *)(scr + 64), et->ph, et->la);
        }
        lds_barrier();
        if (mul) {
            const int lane = lane_id(), lr = lane & 15, lk = lane >> 4;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int orow = wave * 16 + lk + 4 * q, col = 16 * j + lr;
                    if (orow < M && col < na) {
                        const cplx v = cmake(P1[j][q], P2[j][q]);
                        phi_l[orow * nt + col] = v;
                        phi_l[orow * nt + na + col] = v;
                    }
                }
        }
        et->on = true;
        return;
    }
    // ---- closing one-body pass on the alpha half, stored to both spin blocks: beta is the stored copy of alpha
    if (mul) {
        d4_t P1[2], P2[2];
        double bh[KS];
        load_b(bh);
        one_body(cur, bh, P1, P2);
        const int lane = lane_id(), lr = lane & 15, lk = lane >> 4;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int orow = wave * 16 + lk + 4 * q, col = 16 * j + lr;
                if (orow < M && col < na) {
                    const cplx v = cmake(P1[j][q], P2[j][q]);
                    phi[(long)orow * nt + col] = v;
                    phi[(long)orow * nt + na + col] = v;
                }
            }
    }
}
