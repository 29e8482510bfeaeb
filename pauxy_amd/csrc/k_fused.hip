// Fused per-walker propagator:   phi <- B . [ sum_{n<=order} V^n / n! ] . B . phi
// (propagation/continuous.py:251, :162-171 with :82-111, :258) in ONE launch.
//
// One 512-thread work-group (8 waves) per live walker.  The walker's Slater
// matrix never leaves the CU between the 2 + order + 2 matrix products:
//   * T (the current right-hand operand, M x (na+nb) complex) lives in LDS in
//     MFMA B-fragment order: [k-chunk of 8][column-tile slot a0 a1 b0 b1][sub-step][64 lanes x 16 B]
//   * the running Taylor sum lives in registers (waves 0-3 own 2 x 2 tiles, waves 4-7 own 3 x 1: 7 per SIMD;
//     for M <= 100 the third tile of waves 4-7 is one v_mfma_f64_4x4x4 unit of 4 rows x 16 columns instead)
//   * the left operands (BH1[0], BH1[1], VHS[w] x order, BH1[0], BH1[1]) stream through a
//     3-slot LDS ring as ONE continuous sequence of k-chunks filled by global_load_lds
//     (A-fragment order), so the pipeline never drains between products
//   * complex products use the 3-multiplication form (see mfma_gemm_wg.h); when BH1 has no imaginary part
//     (real trial and real Cholesky vectors: the usual case) the four one-body products need only the two
//     real-by-complex multiplications
//   * shapes whose tile deal has no holes (template FULL) run a half-chunk pipeline in which every non-MFMA
//     instruction -- ring refill, fragment reads, address arithmetic -- sits between two MFMA groups of the
//     same wave; the other shapes run a generic loop with per-tile validity tests
//   * a closed-shell walker of the headline's shape class leaves this body right behind the closedness check for the one of
//     k_fused_closed.h: V loaded once into registers, no ring in the Taylor products
// One raw s_barrier per k-chunk; two more per product to hand the result back into T.
// Replaces 2 x 2 one-body launches + order Taylor launches + 3 copy kernels + the
// phi ping-pong buffers of the unfused path; dead walkers (qmc/afqmc.py:232) are skipped
// in place.
// Limits: M <= 104 (13 chunks of T = 104 KB of LDS), na, nb <= 32, one VHS matrix per walker.
#include <cstdlib>
#include <type_traits>

#include "mfma_gemm_wg.h"
#include "greens_small.h"

#define PF_D 3
// waves per work-group: 8 (product) or 16 (experiment: -DPF_NW=16; four waves per SIMD, 2 x 1 tile deals)
#ifndef PF_NW
#define PF_NW 8
#endif
#define PF_NT (64 * PF_NW)
// waves that refill the operand ring: all of them (PF_LW == PF_NW: two fragments per wave and chunk), or the last PF_LW.
// Measured NEGATIVE (round 4, C3): PF_LW = 4 -- waves 4-7, the lighter half of the contiguous-column deal, issuing four
// LDS-DMA instructions per chunk each so that the waves with the 2 x 2 tile blocks never stall in DMA issue -- 149.3 us
// against 140.2 us: four back-to-back DMA instructions hold a wave for several hundred cycles and the chunk barrier makes
// everybody wait for it.
#ifndef PF_LW
#define PF_LW PF_NW
#endif
#define PF_FPW (16 / PF_LW)      // operand fragments each refilling wave moves per chunk

struct PropFusedArgs {
    int M, na, nb, nt, order;
    int vhs_upper;              // vhs holds only the upper triangle of the (symmetric) HS potential
    int same_b;                 // BH1[0] == BH1[1]: one one-body pass serves both spins
    int b_real;                 // BH1 is real: one-body products take 2 real multiplications instead of 3
    int rem4;                   // M <= 100 in the full 7-row-tile deal: rows 96.. as one 4x4x4 unit (see taylor)
    int hyb;                    // with contig: the fourth column slot's at most 4 * hyb <= 8 live columns are multiplied as
                                // hyb units of 16 rows x 4 columns on v_mfma_f64_4x4x4 (see taylor_h)
    int symcols;                // contig with na == nb (round 5): T holds the walker's columns in the order [a 0..15 | b 0..15 |
                                // a 16..23, b 16..23 | a 24.., b 24..] so that a column and its twin of the other spin always go
                                // through the same code and MFMA shape (slots 0, 1: taylor; slot 2: taylor_h's tile; slot 3:
                                // 4x4x4 units): the spin blocks of a closed-shell walker stay bitwise equal through the step
    int closed_try;             // one matrix for both spins, na == nb, a deal without holes: a walker whose spin blocks are bitwise
                                // equal (checked in the kernel, every launch) takes the closed-shell deal of the Taylor products
    int contig;                 // the columns of T are the na + nb columns of the walker back to back (slot = column / 16)
                                // instead of two slots per spin: every matrix of the chain acts on both spins alike
    const cplx *BH1;            // [2, M, M]
    const cplx *vhs;            // [nw, M, M]
    cplx *phi;                  // [nw, M, nt], updated in place
    const int *alive;
    const void *zero16;
    unsigned long long *n_closed;   // afq_counters [3]: walkers that took the closed-shell deal
    int resident;               // a walker found closed takes the body with V resident in registers (k_fused_closed.h)
};

__device__ inline d2_t lds_read_c(unsigned addr) { return lds_read_b128(addr); }

// ds_read_b128 of fragment `idx` (1 KB apart) behind one base register: the offset goes into the instruction,
// so a set of fragment reads costs one address register instead of one per fragment.
template <int OFF> __device__ inline d2_t lds_read_off(unsigned addr) {
    d2_t v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}
__device__ __attribute__((always_inline)) inline d2_t lds_read_frag(unsigned base, int idx) {
    switch (idx) {
    case 0: return lds_read_off<0>(base);
    case 1: return lds_read_off<1024>(base);
    case 2: return lds_read_off<2048>(base);
    case 3: return lds_read_off<3072>(base);
    case 4: return lds_read_off<4096>(base);
    case 5: return lds_read_off<5120>(base);
    case 6: return lds_read_off<6144>(base);
    default: return lds_read_off<7168>(base);
    }
}

// Real part only (ds_read_b64) of fragment `idx`: the operand of a real matrix.  Reading the full 16 bytes and dropping the
// upper half is not equivalent: the register allocator then lets that dead upper half overlap registers an MFMA issued
// shortly before still has to read (measured: wrong rows in the column-deal one-body pass, varying from run to run).
template <int OFF> __device__ inline double lds_read_re_off(unsigned addr) {
    double v;
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}
__device__ __attribute__((always_inline)) inline double lds_read_frag_re(unsigned base, int idx) {
    switch (idx) {
    case 0: return lds_read_re_off<0>(base);
    case 1: return lds_read_re_off<1024>(base);
    case 2: return lds_read_re_off<2048>(base);
    case 3: return lds_read_re_off<3072>(base);
    case 4: return lds_read_re_off<4096>(base);
    case 5: return lds_read_re_off<5120>(base);
    case 6: return lds_read_re_off<6144>(base);
    default: return lds_read_re_off<7168>(base);
    }
}

// Work-group barrier that orders LDS traffic only.  __syncthreads() also waits for vmcnt(0), i.e. for every
// operand chunk still in flight in the DMA ring -- a full pipeline drain at each product boundary.
__device__ inline void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// The step hand-over of the 3-multiplication tail kernel (afq_set_step_handover; afq_handle::handover owns its validity):
// a walker of the EARLY resident body leaves the opening pass of its NEXT step behind, and starts from the one the launch
// before left.  Passed to that kernel alone, by value, behind its other arguments.
struct StepHandoverArgs {
    unsigned char *t0_next;     // [nw][KS * 2048 B] T_0 = B phi' as the resident body's image of T (B-fragment order)
    int *ready;                 // [nw] written for EVERY walker of EVERY launch: 1 = t0_next[w] is the walker's, made by this launch
    const double *B2;           // Re(BH1[0]) . Re(BH1[0]), [M, M] real (host-made)
    unsigned long long *n_handed;   // afq_counters_ext [9]
    int consume;                // the host holds the last launch's hand-over current: a walker whose flag is set starts from it
    int produce;                // EARLY walkers make the next one
};

#include "k_fused_closed.h"

// NARROW: at most one column tile per spin (na, nb <= 16); a separate instantiation so that each carries only the
// Taylor tile deals it uses (register allocation and code size of one variant do not tax the other)
// FULL = number of row tiles when every tile of the deal exists (wide: 5-7 row tiles, i.e. 64 < M <= 112 capped by the
// M <= 104 of the kernel, and na, nb > 16; narrow: 6 row tiles; host-checked), else 0: the per-tile validity tests,
// which cost a branch per tile and k-step inside the MFMA blocks, are compiled out.
// The statements of the kernel are in k_fused_body.h, which the kernel with the Green's function tail (below) includes too.
template <bool NARROW, int FULL>
__global__ __launch_bounds__(PF_NT) void prop_fused_kernel(PropFusedArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr bool MUL3 = false;
#define PF_LEAVE(stored_closed_) return
#define PF_HANDOVER
#define PF_RESIDENT(KS_) prop_closed_resident<KS_, MUL3>(a, smem, phi, vhs)
#include "k_fused_body.h"
#undef PF_RESIDENT
#undef PF_HANDOVER
#undef PF_LEAVE
}

// The same with the step's closing Green's function as its tail (a step of the resident shape class, see step_fuses in
// afq_api.hip): behind whichever body the walker took -- or none, a dead walker's overlap is evaluated like any other -- every
// wave waits for its stores of phi, one barrier makes them the work-group's, and greens_small_body runs on the same dynamic
// LDS: the walker's new phi, both overlap matrices, their inverses, Ghalf (its spin sum alone on an announced step) and the
// weight update where the shift is known, as greens_small_kernel<true, true> with the same arguments would leave them.  A
// walker of the resident body is closed by construction (one result stored to both spin blocks) and skips the tail's compare.
// A separate overload, not a flag of the kernel above: that one keeps its signature, its code and its registers.
// psiB (MUL3 alone; null: off): psi^H B [na, M], real -- afq_set_step_tail_overlap.  A walker of the resident body then has its
// overlap matrix multiplied from the Taylor sum ahead of the closing one-body pass and inverted by wave 7 under it
// (k_fused_closed.h), and the tail starts at its phase 3.  Every other walker of the launch, and every walker with psiB
// null, runs the statements it ran before.
template <bool NARROW, int FULL, bool TAIL, bool MUL3>
__global__ __launch_bounds__(PF_NT) void prop_fused_kernel(PropFusedArgs a, GreensArgs ga, WeightArgs wa, const double *psiB) {
    static_assert(TAIL && !NARROW && FULL == 7, "the tail rides on the full wide deal only");
    static_assert(!MUL3, "the 3-multiplication tail kernel takes the step hand-over: the overload below");
    extern __shared__ __align__(16) unsigned char smem[];
    bool stored_closed = false;
    do {
#define PF_LEAVE(stored_closed_) { stored_closed = (stored_closed_); break; }
#define PF_HANDOVER
#define PF_RESIDENT(KS_) prop_closed_resident<KS_, false>(a, smem, phi, vhs)
#include "k_fused_body.h"
#undef PF_RESIDENT
#undef PF_HANDOVER
#undef PF_LEAVE
    } while (0);
    // the tail's addressing starts from here: nothing of it may be computed (and held in registers) across the bodies above
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
    int w = blockIdx.x;
    asm volatile("" : "+s"(w));
    greens_small_body<true, true>(ga, wa, w, smem, stored_closed);
}

// The 3-multiplication tail kernel: the same, with the early overlap (psiB) and the step hand-over (ho).  An overload by its
// argument list, under the same name: the 4-multiplication tail kernel above keeps its signature, its code and its registers.
// PF_HANDOVER (k_fused_body.h, ahead of everything that reads the walker): when the host holds the hand-over current
// (ho.consume) and the launch before set this walker's flag, the walker is closed by construction and goes straight to the
// EARLY resident body, which then starts at its Taylor products -- through the ONE call of that body this kernel has
// (a run-time flag of the call, not a second copy of the unrolled products).
// ho.ready[w] is written for every walker of every launch, by one lane, behind the bodies: 1 exactly when the walker went
// through the EARLY body with ho.produce set; a dead, an open-shell or a streamed walker clears it.
template <bool NARROW, int FULL, bool TAIL, bool MUL3>
__global__ __launch_bounds__(PF_NT) void prop_fused_kernel(PropFusedArgs a, GreensArgs ga, WeightArgs wa, const double *psiB,
                                                           StepHandoverArgs ho) {
    static_assert(TAIL && !NARROW && FULL == 7 && MUL3, "the tail rides on the full wide deal only");
    extern __shared__ __align__(16) unsigned char smem[];
    bool stored_closed = false;
    EarlyTail early;
    early.on = false;
    do {
#define PF_LEAVE(stored_closed_) { stored_closed = (stored_closed_); break; }
#define PF_HANDOVER                                                                                           \
    if (ho.consume) {                                                                                         \
        handed = __builtin_amdgcn_readfirstlane(ho.ready[w]) != 0;                                            \
        if (handed && threadIdx.x == 0) { atomicAdd(a.n_closed, 1ULL); atomicAdd(ho.n_handed, 1ULL); }        \
    }
#define PF_RESIDENT(KS_)                                                                                      \
    do {                                                                                                      \
        if (psiB) prop_closed_resident<KS_, true, true>(a, smem, phi, vhs, psiB, &early, &ho, handed);        \
        else prop_closed_resident<KS_, true>(a, smem, phi, vhs);                                              \
    } while (0)
#include "k_fused_body.h"
#undef PF_RESIDENT
#undef PF_HANDOVER
#undef PF_LEAVE
    } while (0);
    if (ho.ready && threadIdx.x == 0) ho.ready[blockIdx.x] = (early.on && ho.produce) ? 1 : 0;
    // the tail's addressing starts from here: nothing of it may be computed (and held in registers) across the bodies above
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
    int w = blockIdx.x;
    asm volatile("" : "+s"(w));
    greens_small_body<true, true, true>(ga, wa, w, smem, stored_closed, &early);
}

int k_prop_fused_supported(afq_handle *h) {
    return !h->vhs_diag && h->nv == 1 && h->M <= 104 && h->na <= 32 && h->nb <= 32 && h->nb > 0;
}

// Shape class of the closed-shell body with V resident in registers (k_fused_closed.h), and the form the handle asks for
// (afq_set_propagator_closed_form): closed walkers of any other shape, and all of them in mode 1, take the streamed deal.
int k_prop_closed_resident(afq_handle *h) {
    // LDS of the body against the launch's (k_prop_fused): both images of T, psi^H B as A fragments (1 KB per k-step) and the
    // three partial products of the split deal (4 KB each); a shape that did not fit would take the streamed deal
    const size_t KS = (h->M + 3) / 4, NCH = (h->M + 7) / 8;
    if (KS * (2 * 2048 + 1024) + 3 * 4096 > NCH * 8192 + (size_t)PF_D * 16384) return 0;
    return PF_NW == 8 && k_prop_fused_supported(h) && h->prop_closed_mode != 1 && h->bh1_same && h->bh1_real &&
           h->na == h->nb && h->na > 16 && h->na <= 32 && h->M > 96 && h->M <= 104 && h->exp_order > 0;
}

// Shape class of the announced steps that run their closing Green's function as the propagator's tail: the resident class,
// with the tail's LDS image (greens_fill's size: both overlap matrices, their inverses, the walker) inside the propagator's own
int k_step_fusion_shape(afq_handle *h) {
    if (!k_prop_closed_resident(h)) return 0;
    const size_t nmax = h->na, NCH = (h->M + 7) / 8;
    const size_t tail = sizeof(cplx) * (2 * (nmax * nmax + 2 * nmax) + ((2 * nmax + 3) / 4 + 1) + (size_t)h->M * h->nt);
    return tail <= NCH * 8192 + (size_t)PF_D * 16384;
}

int k_prop_fused(afq_handle *h, const GreensLaunch *tail, bool mul3) {
    PropFusedArgs a;
    a.M = h->M; a.na = h->na; a.nb = h->nb; a.nt = h->nt; a.order = h->exp_order;
    a.vhs_upper = h->vhs_upper ? 1 : 0;
    a.same_b = h->bh1_same ? 1 : 0;
    a.b_real = h->bh1_real ? 1 : 0;
    a.rem4 = (h->M > 96 && h->M <= 100) ? 1 : 0;
    // (hybrid column tiling of the two-slots-per-spin layout -- both spins with 17 .. 28 electrons, their second slots as
    //  4-column units -- measured NEGATIVE at C3, round 4: 148.6 us against 145.5 us -- three 4x4x4 units need 9 MFMA + 3 add
    //  instructions where the padded 16x16x4 tile needs 3 + 1, and a wave that multiplies mostly units is bound by
    //  instruction issue, not by the matrix pipe)
    a.hyb = 0;
    // contiguous columns: one one-body matrix for both spins (the HS potential never depends on the spin), 48 < na + nb <= 56
    // (a third unit per row tile would unbalance the deal and push wave 7 over 256 registers)
    a.contig = 0; a.symcols = 0;
    if (a.rem4 && a.same_b && h->na > 16 && h->nb > 16 && h->nt > 48 && h->nt <= 56 && PF_NW == 8) {
        a.contig = 1;
        a.hyb = (h->nt - 48 + 3) / 4;
    }
    a.symcols = (a.contig && h->na == h->nb) ? 1 : 0;
    a.closed_try = 0;           // (set below, once the deal is known)
    a.BH1 = h->BH1; a.vhs = h->vhs; a.phi = h->phi; a.alive = h->alive; a.zero16 = h->zero_page;
    a.n_closed = h->counters + 3;
    const int NCH = (h->M + 7) / 8;
    const size_t lds = (size_t)NCH * 8192 + (size_t)PF_D * 16384;
    static size_t lds_set[8][AFQ_MAX_DEVICES] = {{0}, {0}, {0}, {0}, {0}, {0}, {0}, {0}};
    const bool narrow = h->na <= 16 && h->nb <= 16;
    // the overlap matrix and its inverse under the closing pass of the resident body (afq_set_step_tail_overlap): the
    // 3-multiplication tail of a step whose closed walkers take the tail's one-spin path against a real trial -- psiB_cT exists
    // for such a trial and one real one-body matrix only (afq_api.hip)
    const bool early = tail && mul3 && h->step_tail_overlap && h->psiB_cT && k_prop_closed_resident(h) &&
                       tail->a.psi_real && tail->a.psi_closed && tail->a.psi_stride == 0 &&
                       (const void *)tail->a.psi == h->psiB_psi && (const void *)h->BH1 == h->psiB_bh1 &&
                       tail->a.gsum && tail->a.ghalf && !tail->a.oinv;
    // The step hand-over (afq_handle::handover): what the launch before left is taken only when the host still holds it current
    // and this launch is the kernel that made it; whatever this launch turns out to be, the old one is gone with it.
    const bool consumes = early && h->handover.current && h->handover.enabled && h->t0_next && h->t0_ready;
    h->handover.drop();
    const bool produces = early && h->step_handover && h->handover.enabled && h->B2 && (const void *)h->BH1 == h->b2_bh1;
    if (produces && (!h->t0_next || !h->t0_ready)) {
        AFQ_TRY(dev_alloc(h, LT_WALKERS, &h->t0_next, (size_t)h->nw * ((h->M + 3) / 4) * 2048, "step hand-over image"));
        AFQ_TRY(dev_alloc(h, LT_WALKERS, &h->t0_ready, (size_t)h->nw, "step hand-over flags"));
    }
    KernelTrace kt(h, AFQ_K_PROPAGATOR);
    {   // matrix-pipe flops of this launch: (order complex products by 3 multiplications + 2 one-body applications by 2 or
        // 3) x k-steps of 4 x existing 16 x 16 tiles (2048 flop per v_mfma_f64_16x16x4, 512 per 4x4x4 remainder unit)
        const int nrt_ = (h->M + 15) / 16, ct = (h->na + 15) / 16 + (h->nb + 15) / 16;
        const double ksteps = 2.0 * NCH;
        const double per_pass = ksteps * (2048.0 * (a.rem4 ? nrt_ - 1 : nrt_) * ct + 512.0 * (a.rem4 ? ct : 0));
        // contiguous columns: three full slots + hyb units per row tile in the Taylor products, four remainder units in all
        const double taylor_pass = a.contig ? ksteps * (2048.0 * (nrt_ - 1) * 3 + 512.0 * (nrt_ - 1) * a.hyb + 512.0 * 4) : per_pass;
        h->issued_flops[AFQ_K_PROPAGATOR] = (3.0 * h->exp_order * taylor_pass + 2.0 * (a.b_real ? 2.0 : 3.0) * per_pass) * h->nw;
        h->prop_issued_open = h->issued_flops[AFQ_K_PROPAGATOR] / h->nw;
        // a closed-shell walker (afq_counters [3]) issues the alpha slots only in its Taylor products: two column slots x the
        // row tiles (+ two remainder units in the M <= 100 deal), one slot when narrow; its one-body passes multiply every slot.
        // Waves that repeat a tile (five row tiles, narrow) and row tiles that do not exist are not counted, as above
        const int cta = (h->na + 15) / 16;
        const double closed_pass = ksteps * (2048.0 * (a.rem4 ? nrt_ - 1 : nrt_) * cta + 512.0 * (a.rem4 ? cta : 0));
        h->prop_issued_closed = 3.0 * h->exp_order * closed_pass + 2.0 * (a.b_real ? 2.0 : 3.0) * per_pass;
        // ... through the resident body: seven padded row tiles x the two alpha slots x ceil(M / 4) k-steps in every product
        // (4-multiplication Taylor products, two real products in each of the two one-body passes)
        // (the one-body passes the launch really issues: the opening one unless the walkers start from the hand-over, the
        //  closing one, and the next step's opening one where the launch produces -- two in steady state, as without it)
        if (k_prop_closed_resident(h)) {
            const double passes = (consumes ? 0.0 : 1.0) + 1.0 + (produces ? 1.0 : 0.0);
            h->prop_issued_closed = ((tail && mul3 ? 3.0 : 4.0) * h->exp_order + passes * 2.0) * ((h->M + 3) / 4) * 2048.0 * 7 * 2;
        }
        if (tail) {
            // ... and the tail's (greens_small_body, n <= 32): the overlap matrix as (n / 16)^2 tiles per spin over the k-steps of M
            // in whole groups of four, two multiplications per k-step against a real trial, else three; O^-1 phi^T as (n / 16) x
            // (M / 16) tiles per spin over ceil(n / 4) k-steps of three.  A closed walker evaluates one spin.  (The same count
            // whether the tail stores the per-spin Ghalf or not and whether the weight update rides: those are stores and
            // one thread's scalar arithmetic, no MFMA.)
            const double t16 = (h->na + 15) / 16, m16 = (h->M + 15) / 16;
            const double ks1 = 4.0 * (((h->M + 3) / 4 + 3) / 4), ks3 = (h->na + 3) / 4;
            const double spin = 2048.0 * (t16 * t16 * ks1 * (tail->a.psi_real ? 2.0 : 3.0) + t16 * m16 * ks3 * 3.0);
            h->prop_issued_open += 2.0 * spin;
            h->prop_issued_closed += (tail->a.psi_closed ? 1.0 : 2.0) * spin;
            // ... with the overlap matrix made early by the resident body (psi^H B times the Taylor sum: four tiles over the
            // ceil(M / 4) k-steps, two real multiplications each) in place of the tail's own
            if (early) h->prop_issued_closed += 2048.0 * (4.0 * ((h->M + 3) / 4) * 2.0 - t16 * t16 * ks1 * 2.0);
            h->issued_flops[AFQ_K_PROPAGATOR] = h->prop_issued_open * h->nw;
        }
    }
    // every tile of the deal present: wide with 5-7 row tiles (waves 4-7 own the tiles from 4 on) and two column tiles
    // per spin, or narrow with six row tiles
    const int nrt = (h->M + 15) / 16;
    const bool nofull = PF_NW != 8;
    const int full = nofull ? 0 : narrow ? (nrt == 6 ? 6 : 0) : (nrt >= 5 && h->na > 16 && h->nb > 16 ? nrt : 0);
    // closed-shell deals: one matrix for both spins (the chain then acts on the spin blocks alike), as many electrons of
    // either spin, and a deal without holes: the contiguous-column deal with twins in like slots (symcols), or two slots per spin
    a.closed_try = (a.same_b && h->na == h->nb && h->exp_order > 0 && full != 0 && PF_NW == 8 &&
                    (!a.contig || a.symcols)) ? 1 : 0;
    a.resident = (a.closed_try && full == 7 && k_prop_closed_resident(h)) ? 1 : 0;
#define PF_LAUNCH_(NARROW_, FULL_, SLOT_)                                                                     \
    do {                                                                                                      \
        AFQ_HIP(h, afq_raise_lds((const void *)prop_fused_kernel<NARROW_, FULL_>, lds, lds_set[SLOT_]));      \
        AFQ_LAUNCH(h, (prop_fused_kernel<NARROW_, FULL_>), dim3(h->nw), dim3(PF_NT), lds, h->stream, a);      \
    } while (0)
    if (tail) {
        // (afq_propagate has checked the step and k_step_fusion_shape the shape; the launch is named for the propagator it is)
        if (full != 7 || !a.resident || tail->lds > lds)
            AFQ_FAIL(h, AFQ_ESTATE, "internal: a Green's function tail on a propagator launch outside its shape class");
        if (mul3) {
            void (*const kern)(PropFusedArgs, GreensArgs, WeightArgs, const double *, StepHandoverArgs) =
                prop_fused_kernel<false, 7, true, true>;
            AFQ_HIP(h, afq_raise_lds((const void *)kern, lds, lds_set[6]));
            const double *psiB = early ? h->psiB_cT : nullptr;
            StepHandoverArgs ho;
            ho.t0_next = h->t0_next; ho.ready = h->t0_ready; ho.B2 = h->B2; ho.n_handed = h->counters + 9;
            ho.consume = consumes ? 1 : 0; ho.produce = produces ? 1 : 0;
            AFQ_LAUNCH(h, (prop_fused_kernel<false, 7, true, true>), dim3(h->nw), dim3(PF_NT), lds, h->stream, a, tail->a, tail->wa, psiB, ho);
        } else {
            const double *psiB = nullptr;
            void (*const kern)(PropFusedArgs, GreensArgs, WeightArgs, const double *) = prop_fused_kernel<false, 7, true, false>;
            AFQ_HIP(h, afq_raise_lds((const void *)kern, lds, lds_set[7]));
            AFQ_LAUNCH(h, (prop_fused_kernel<false, 7, true, false>), dim3(h->nw), dim3(PF_NT), lds, h->stream, a, tail->a, tail->wa, psiB);
        }
    }
    else if (narrow && full) PF_LAUNCH_(true, 6, 0);
    else if (narrow) PF_LAUNCH_(true, 0, 1);
    else if (full == 7) PF_LAUNCH_(false, 7, 2);
    else if (full == 6) PF_LAUNCH_(false, 6, 3);
    else if (full == 5) PF_LAUNCH_(false, 5, 4);
    else PF_LAUNCH_(false, 0, 5);
#undef PF_LAUNCH_
    AFQ_POST(h);
    if (produces) h->handover.produced();
    return AFQ_OK;
}
