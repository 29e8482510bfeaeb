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
#include "step_plan.h"

#define PF_D 3
// waves per work-group.  (Sixteen -- four waves per SIMD, 2 x 1 tile deals -- ran in the same time as eight, HISTORY.md; that
// variant is no longer in the source.)
#define PF_NW 8
#define PF_NT (64 * PF_NW)
// waves that refill the operand ring: all of them, two fragments per wave and chunk.
// Measured NEGATIVE (round 4, C3): the last four only -- waves 4-7, the lighter half of the contiguous-column deal, issuing four
// LDS-DMA instructions per chunk each so that the waves with the 2 x 2 tile blocks never stall in DMA issue -- 149.3 us
// against 140.2 us: four back-to-back DMA instructions hold a wave for several hundred cycles and the chunk barrier makes
// everybody wait for it (NEGATIVES.md; profiles/r06_prop_fused_loader_deal_experiment.patch).
#define PF_LW PF_NW
#define PF_FPW (16 / PF_LW)      // operand fragments each wave moves per chunk

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

// The same with the step's closing Green's function as its tail (a step of the resident shape class, see k_step_fuses
// below): behind whichever body the walker took -- or none, a dead walker's overlap is evaluated like any other -- every
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

// ---- the host side.  What a launch is, is decided by step_plan() (step_plan.h) from the facts gathered here; the code below
// reads the plan.
static_assert(PF_D == STEP_PLAN_RING, "the plan sizes the launch's LDS for this operand ring");

// The handle as the plan sees it: system, propagator, population, switches (no step, no tail)
static StepFacts step_facts(afq_handle *h) {
    const StepState &st = h->step;
    StepFacts f;
    f.M = h->M; f.na = h->na; f.nb = h->nb; f.nw = h->nw; f.order = h->exp_order;
    f.nv = h->nv; f.vhs_diag = h->vhs_diag; f.same_b = h->bh1_same; f.b_real = h->bh1_real;
    f.closed_mode = st.get(StepState::CLOSED_FORM);
    f.fusion_mode = st.get(StepState::FUSION); f.fusion_scope = st.get(StepState::SCOPE);
    f.tail_overlap = st.get(StepState::TAIL_OVERLAP) != 0; f.handover = st.get(StepState::HANDOVER) != 0;
    return f;
}

int k_prop_fused_supported(afq_handle *h) { return step_plan(step_facts(h)).supported; }
// (the form the handle asks for included, afq_set_propagator_closed_form)
int k_prop_closed_resident(afq_handle *h) { return step_plan(step_facts(h)).resident_class; }

// Whether THIS step runs its closing Green's function (with the overlap and the weight update) as the tail of the fused
// propagator's launch: begin and finish in one call (the weight update needs the energy shift), announced with
// afq_estimates_fuse_next, of the resident closed-shell shape class, and of the kind whose closing evaluation may skip the
// per-spin store (afq_propagate_finish, GreensRequest::may_skip_store) -- the tail leaves overlap + spin sum behind, nothing
// else.  Every other step runs the two launches.
// afq_set_step_fusion_scope(1) drops the first two conditions: an unannounced step's tail stores the per-spin Ghalf too (the
// request afq_propagate_finish would have made), and the tail of a begin without a finish in the same call evaluates Green's
// function and overlap only -- the shift is not known yet -- and leaves the weight update to afq_propagate_finish.
bool k_step_fuses(afq_handle *h) {
    StepFacts f = step_facts(h);
    f.one_call = h->step.one_call;
    f.announced = h->fuse_est_req;
    f.plain_step = h->gf.enabled && h->ndet == 1 && h->kind == AFQ_SYS_GENERIC && (h->flags & AFQ_PROP_HYBRID) &&
                   (h->flags & AFQ_PROP_FORCE_BIAS) && !(h->flags & AFQ_PROP_FREE_PROJECTION) && !h->rdm_on && h->nbp == 0 &&
                   h->psi_stride == 0 && !h->hirsch && !k_greens_big_supported(h) && k_fb_use_sum(h);
    return step_plan(f).fuses;
}

// The eight instantiations, in the order of StepVariant (step_plan.h): the kernel, its breadcrumb / launch-trace name and the
// dynamic-LDS cap raised so far per device.  The kernels differ in their argument lists; every launch passes the same array of
// argument addresses, of which each kernel takes the ones it has.  (The entries stand in the order in which the host code
// instantiated the kernels before there was a table: the device code is emitted in that order.)
typedef void (*PropKernel)(PropFusedArgs);
typedef void (*PropTail4Kernel)(PropFusedArgs, GreensArgs, WeightArgs, const double *);
typedef void (*PropTail3Kernel)(PropFusedArgs, GreensArgs, WeightArgs, const double *, StepHandoverArgs);
struct PropVariant { const void *kern; const char *name; size_t lds_set[AFQ_MAX_DEVICES]; };
#define PROP_VARIANT(type, kern) {(const void *)static_cast<type>(kern), #kern, {0}}
static PropVariant prop_variants[PV_COUNT] = {
    PROP_VARIANT(PropTail3Kernel, (prop_fused_kernel<false, 7, true, true>)),
    PROP_VARIANT(PropTail4Kernel, (prop_fused_kernel<false, 7, true, false>)),
    PROP_VARIANT(PropKernel, (prop_fused_kernel<true, 6>)), PROP_VARIANT(PropKernel, (prop_fused_kernel<true, 0>)),
    PROP_VARIANT(PropKernel, (prop_fused_kernel<false, 7>)), PROP_VARIANT(PropKernel, (prop_fused_kernel<false, 6>)),
    PROP_VARIANT(PropKernel, (prop_fused_kernel<false, 5>)), PROP_VARIANT(PropKernel, (prop_fused_kernel<false, 0>))};
#undef PROP_VARIANT

int k_prop_fused(afq_handle *h, const GreensLaunch *tail, bool mul3) {
    StepState &st = h->step;
    StepFacts f = step_facts(h);
    if (tail) {
        // (afq_propagate has checked the step and k_step_fuses the shape; the launch is named for the propagator it is)
        f.tail = true; f.mul3 = mul3; f.tail_lds = tail->lds;
        f.tail_psi_real = tail->a.psi_real; f.tail_psi_closed = tail->a.psi_closed; f.tail_shared_psi = tail->a.psi_stride == 0;
        f.tail_spin_sum = tail->a.gsum && tail->a.ghalf && !tail->a.oinv;
        f.psiB_ready = st.psiB_ready(tail->a.psi, h->BH1);
    }
    f.B2_ready = st.B2_ready(h->BH1);
    f.handover_enabled = st.handover.enabled; f.handover_current = st.handover_current();
    const StepPlan p = step_plan(f);
    st.handover.drop();             // whatever this launch turns out to be, the hand-over of the launch before is gone with it
    if (p.produces && (!st.t0_next || !st.t0_ready)) {
        AFQ_TRY(dev_alloc(h, LT_WALKERS, &st.t0_next, (size_t)h->nw * ((h->M + 3) / 4) * 2048, "step hand-over image"));
        AFQ_TRY(dev_alloc(h, LT_WALKERS, &st.t0_ready, (size_t)h->nw, "step hand-over flags"));
    }
    st.issued = plan_issued_flops(p);
    h->issued_flops[AFQ_K_PROPAGATOR] = st.issued.total;
    if (p.refusal) AFQ_FAIL(h, AFQ_ESTATE, p.refusal);

    PropFusedArgs a;
    a.M = h->M; a.na = h->na; a.nb = h->nb; a.nt = h->nt; a.order = h->exp_order;
    a.vhs_upper = st.vhs_upper ? 1 : 0;
    a.same_b = f.same_b ? 1 : 0; a.b_real = f.b_real ? 1 : 0;
    a.rem4 = p.rem4; a.hyb = p.hyb; a.symcols = p.symcols; a.closed_try = p.closed_try; a.contig = p.contig;
    a.BH1 = h->BH1; a.vhs = h->vhs; a.phi = h->phi; a.alive = h->alive; a.zero16 = h->zero_page;
    a.n_closed = h->counters + 3;
    a.resident = p.resident;
    const double *psiB = p.early ? st.psiB_cT : nullptr;
    StepHandoverArgs ho;
    ho.t0_next = st.t0_next; ho.ready = st.t0_ready; ho.B2 = st.B2; ho.n_handed = h->counters + 9;
    ho.consume = p.consumes ? 1 : 0; ho.produce = p.produces ? 1 : 0;
    void *args[] = {&a, tail ? (void *)&tail->a : nullptr, tail ? (void *)&tail->wa : nullptr, &psiB, &ho};

    KernelTrace kt(h, AFQ_K_PROPAGATOR);
    PropVariant &v = prop_variants[p.variant];
    AFQ_HIP(h, afq_raise_lds(v.kern, p.lds, v.lds_set));
    afq_note_launch(h, v.name);
    (void)hipLaunchKernel(v.kern, dim3(h->nw), dim3(PF_NT), args, p.lds, h->stream);      // (AFQ_POST reads the launch's error)
    AFQ_POST(h);
    if (p.produces) st.handover.produced();
    return AFQ_OK;
}
