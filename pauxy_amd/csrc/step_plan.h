// What ONE launch of the fused propagator (k_fused.hip) is: decided here, from plain facts, and nowhere else.
//
// step_plan(facts) is the only place that chooses the tile deal, the shape class, the tail (none, behind the 4-multiplication
// body, behind the 3-multiplication one), the early overlap, what the launch takes from and leaves for the step hand-over,
// the instantiation and the dynamic LDS -- and whether a step runs its closing Green's function as that tail at all.
// plan_issued_flops(plan) counts the matrix-pipe flops of exactly that launch.  The host code around the kernels reads the
// plan: k_prop_fused fills the arguments from it, the predicates (k_prop_fused_supported, k_prop_closed_resident,
// k_step_fuses) are reads of it, and a launch the plan refuses is an internal error.
// Plain C++: no HIP header, no handle, no allocation (tests/step_plan_main.cpp builds it with the host compiler alone).
#pragma once
#include <cstddef>

// PF_D: slots of the operand ring (16 KB each) behind the chunks of T (8 KB each) in the launch's dynamic LDS
constexpr int STEP_PLAN_RING = 3;

struct StepFacts {
    // ---- the system, the propagator, the population
    int M = 0, na = 0, nb = 0, nw = 0, order = 0;
    int nv = 1;                     // HS matrices per walker
    bool vhs_diag = false;          // ... stored as diagonals (Hubbard)
    bool same_b = false;            // BH1[0] == BH1[1], bitwise
    bool b_real = false;            // BH1 has no imaginary part
    // ---- the switches (StepState, step_state.h)
    int closed_mode = 0;            // afq_set_propagator_closed_form
    int fusion_mode = 2;            // afq_set_step_fusion
    int fusion_scope = 0;           // afq_set_step_fusion_scope
    bool tail_overlap = true;       // afq_set_step_tail_overlap
    bool handover = true;           // afq_set_step_handover
    // ---- the step: one call with the shift known, announced with afq_estimates_fuse_next, and of the kind whose closing
    // evaluation is the small kernel's with the spin sum (hybrid, force bias, one determinant, no window, no one_rdm, ...)
    bool one_call = false, announced = false, plain_step = false;
    // ---- the tail this launch carries (k_prop_fused_greens has filled it), or none
    bool tail = false, mul3 = false;
    size_t tail_lds = 0;
    bool tail_psi_real = false, tail_psi_closed = false;
    bool tail_shared_psi = false;   // one trial for every walker
    bool tail_spin_sum = false;     // stores Ghalf and its spin sum, not O^-1
    // ---- the host-made operands and the hand-over buffers (StepState)
    bool psiB_ready = false;        // psi^H B exists and was made of the tail's trial and this propagator
    bool B2_ready = false;          // B B exists and was made of this propagator
    bool handover_enabled = true;   // no device pointer to phi was handed out
    bool handover_current = false;  // the buffers exist and describe the walkers as they are now
};

enum StepTail { STEP_TAIL_NONE = 0, STEP_TAIL_MUL4, STEP_TAIL_MUL3 };

// The eight instantiations of prop_fused_kernel, in the order of the launch table of k_fused.hip
enum StepVariant {
    PV_TAIL_MUL3 = 0, PV_TAIL_MUL4, PV_NARROW_FULL, PV_NARROW, PV_WIDE_7, PV_WIDE_6, PV_WIDE_5, PV_WIDE, PV_COUNT
};
inline const char *step_variant_name(int v) {
    static const char *const names[PV_COUNT] = {
        "(prop_fused_kernel<false, 7, true, true>)", "(prop_fused_kernel<false, 7, true, false>)",
        "(prop_fused_kernel<true, 6>)", "(prop_fused_kernel<true, 0>)", "(prop_fused_kernel<false, 7>)",
        "(prop_fused_kernel<false, 6>)", "(prop_fused_kernel<false, 5>)", "(prop_fused_kernel<false, 0>)"};
    return v >= 0 && v < PV_COUNT ? names[v] : "";
}

struct StepPlan {
    StepFacts f;                    // what it was made of
    bool supported = false;         // the fused propagator serves the shape at all
    bool resident_class = false;    // closed walkers take the body with V resident in registers (k_fused_closed.h)
    bool fusion_shape = false;      // ... and the tail's LDS image fits inside the propagator's own
    bool fuses = false;             // THIS step runs its closing Green's function as the tail
    // ---- the deal (PropFusedArgs of the same names)
    bool narrow = false;            // at most one column tile per spin
    int full = 0;                   // row tiles when every tile of the deal exists, else 0
    int rem4 = 0, hyb = 0, contig = 0, symcols = 0, closed_try = 0, resident = 0;
    StepTail tail = STEP_TAIL_NONE;
    bool early = false;             // the tail's overlap matrix and inverse under the resident body's closing pass
    bool consumes = false;          // resident walkers start from the hand-over of the launch before
    bool produces = false;          // ... and leave the next step's
    int variant = PV_WIDE;
    size_t lds = 0;                 // dynamic LDS of the launch
    const char *refusal = nullptr;  // the launch as asked for is outside its shape class (an internal error), or null
};

struct StepFlops { double open = 0.0, closed = 0.0, total = 0.0; };    // per open walker, per closed walker, the launch

inline StepPlan step_plan(const StepFacts &f) {
    StepPlan p;
    p.f = f;
    const int M = f.M, na = f.na, nb = f.nb, nt = f.na + f.nb;
    const size_t NCH = (M + 7) / 8, KS = (M + 3) / 4;
    p.lds = NCH * 8192 + (size_t)STEP_PLAN_RING * 16384;
    p.supported = !f.vhs_diag && f.nv == 1 && M <= 104 && na <= 32 && nb <= 32 && nb > 0;
    // the resident body's LDS against the launch's: both images of T, psi^H B as A fragments (1 KB per k-step) and the three
    // partial products of the split deal (4 KB each); closed walkers of any other shape, and all of them in mode 1, take the
    // streamed deal
    p.resident_class = KS * (2 * 2048 + 1024) + 3 * 4096 <= p.lds && p.supported && f.closed_mode != 1 && f.same_b &&
                       f.b_real && na == nb && na > 16 && na <= 32 && M > 96 && M <= 104 && f.order > 0;
    // the tail's LDS image (greens_fill's size: both overlap matrices, their inverses, the walker) inside the propagator's own
    const size_t nmax = na;
    p.fusion_shape = p.resident_class &&
                     16 * (2 * (nmax * nmax + 2 * nmax) + ((2 * nmax + 3) / 4 + 1) + (size_t)M * nt) <= p.lds;
    p.fuses = (f.fusion_scope == 1 || (f.one_call && f.announced)) && f.fusion_mode != 0 && f.plain_step && p.fusion_shape;
    if (!p.supported) return p;

    // ---- the deal
    p.rem4 = (M > 96 && M <= 100) ? 1 : 0;
    // (hybrid column tiling of the two-slots-per-spin layout -- both spins with 17 .. 28 electrons, their second slots as
    //  4-column units -- measured NEGATIVE at C3, round 4: 148.6 us against 145.5 us -- three 4x4x4 units need 9 MFMA + 3 add
    //  instructions where the padded 16x16x4 tile needs 3 + 1, and a wave that multiplies mostly units is bound by
    //  instruction issue, not by the matrix pipe)
    // contiguous columns: one one-body matrix for both spins (the HS potential never depends on the spin), 48 < na + nb <= 56
    // (a third unit per row tile would unbalance the deal and push wave 7 over 256 registers)
    if (p.rem4 && f.same_b && na > 16 && nb > 16 && nt > 48 && nt <= 56) {
        p.contig = 1;
        p.hyb = (nt - 48 + 3) / 4;
    }
    p.symcols = (p.contig && na == nb) ? 1 : 0;
    p.narrow = na <= 16 && nb <= 16;
    // every tile of the deal present: wide with 5-7 row tiles (waves 4-7 own the tiles from 4 on) and two column tiles
    // per spin, or narrow with six row tiles
    const int nrt = (M + 15) / 16;
    p.full = p.narrow ? (nrt == 6 ? 6 : 0) : (nrt >= 5 && na > 16 && nb > 16 ? nrt : 0);
    // closed-shell deals: one matrix for both spins (the chain then acts on the spin blocks alike), as many electrons of
    // either spin, and a deal without holes: the contiguous-column deal with twins in like slots (symcols), or two slots per spin
    p.closed_try = (f.same_b && na == nb && f.order > 0 && p.full != 0 && (!p.contig || p.symcols)) ? 1 : 0;
    p.resident = (p.closed_try && p.full == 7 && p.resident_class) ? 1 : 0;

    // ---- the tail, the early overlap, the hand-over
    p.tail = !f.tail ? STEP_TAIL_NONE : f.mul3 ? STEP_TAIL_MUL3 : STEP_TAIL_MUL4;
    if (f.tail && (p.full != 7 || !p.resident || f.tail_lds > p.lds))
        p.refusal = "internal: a Green's function tail on a propagator launch outside its shape class";
    // the overlap matrix and its inverse under the closing pass of the resident body: the 3-multiplication tail of a step
    // whose closed walkers take the tail's one-spin path against a real trial
    p.early = p.tail == STEP_TAIL_MUL3 && f.tail_overlap && f.psiB_ready && p.resident_class && f.tail_psi_real &&
              f.tail_psi_closed && f.tail_shared_psi && f.tail_spin_sum;
    // what the launch before left is taken only when the host still holds it current and this launch is the kernel that made it
    p.consumes = p.early && f.handover_current && f.handover_enabled;
    p.produces = p.early && f.handover && f.handover_enabled && f.B2_ready;
    p.variant = p.tail == STEP_TAIL_MUL3 ? PV_TAIL_MUL3 : p.tail == STEP_TAIL_MUL4 ? PV_TAIL_MUL4 :
                p.narrow ? (p.full ? PV_NARROW_FULL : PV_NARROW) :
                p.full == 7 ? PV_WIDE_7 : p.full == 6 ? PV_WIDE_6 : p.full == 5 ? PV_WIDE_5 : PV_WIDE;
    return p;
}

// Matrix-pipe flops of the planned launch: (order complex products by 3 multiplications + 2 one-body applications by 2 or 3)
// x k-steps of 4 x existing 16 x 16 tiles (2048 flop per v_mfma_f64_16x16x4, 512 per 4x4x4 remainder unit)
inline StepFlops plan_issued_flops(const StepPlan &p) {
    const StepFacts &f = p.f;
    StepFlops out;
    const int M = f.M, na = f.na, nb = f.nb, NCH = (M + 7) / 8;
    const int nrt = (M + 15) / 16, ct = (na + 15) / 16 + (nb + 15) / 16;
    const double ksteps = 2.0 * NCH, onebody = 2.0 * (f.b_real ? 2.0 : 3.0);
    const double per_pass = ksteps * (2048.0 * (p.rem4 ? nrt - 1 : nrt) * ct + 512.0 * (p.rem4 ? ct : 0));
    // contiguous columns: three full slots + hyb units per row tile in the Taylor products, four remainder units in all
    const double taylor_pass = p.contig ? ksteps * (2048.0 * (nrt - 1) * 3 + 512.0 * (nrt - 1) * p.hyb + 512.0 * 4) : per_pass;
    out.total = (3.0 * f.order * taylor_pass + onebody * per_pass) * f.nw;
    out.open = out.total / f.nw;
    // a closed-shell walker (afq_counters [3]) issues the alpha slots only in its Taylor products: two column slots x the
    // row tiles (+ two remainder units in the M <= 100 deal), one slot when narrow; its one-body passes multiply every slot.
    // Waves that repeat a tile (five row tiles, narrow) and row tiles that do not exist are not counted, as above
    const int cta = (na + 15) / 16;
    const double closed_pass = ksteps * (2048.0 * (p.rem4 ? nrt - 1 : nrt) * cta + 512.0 * (p.rem4 ? cta : 0));
    out.closed = 3.0 * f.order * closed_pass + onebody * per_pass;
    // ... through the resident body: seven padded row tiles x the two alpha slots x ceil(M / 4) k-steps in every product
    // (4-multiplication Taylor products, 3 behind the 3-multiplication tail; two real products in each one-body pass)
    // (the one-body passes the launch really issues: the opening one unless the walkers start from the hand-over, the
    //  closing one, and the next step's opening one where the launch produces -- two in steady state, as without it)
    if (p.resident_class) {
        const double passes = (p.consumes ? 0.0 : 1.0) + 1.0 + (p.produces ? 1.0 : 0.0);
        out.closed = ((p.tail == STEP_TAIL_MUL3 ? 3.0 : 4.0) * f.order + passes * 2.0) * ((M + 3) / 4) * 2048.0 * 7 * 2;
    }
    if (p.tail != STEP_TAIL_NONE) {
        // ... and the tail's (greens_small_body, n <= 32): the overlap matrix as (n / 16)^2 tiles per spin over the k-steps of M
        // in whole groups of four, two multiplications per k-step against a real trial, else three; O^-1 phi^T as (n / 16) x
        // (M / 16) tiles per spin over ceil(n / 4) k-steps of three.  A closed walker evaluates one spin.  (The same count
        // whether the tail stores the per-spin Ghalf or not and whether the weight update rides: those are stores and
        // one thread's scalar arithmetic, no MFMA.)
        const double t16 = (na + 15) / 16, m16 = (M + 15) / 16;
        const double ks1 = 4.0 * (((M + 3) / 4 + 3) / 4), ks3 = (na + 3) / 4;
        const double spin = 2048.0 * (t16 * t16 * ks1 * (f.tail_psi_real ? 2.0 : 3.0) + t16 * m16 * ks3 * 3.0);
        out.open += 2.0 * spin;
        out.closed += (f.tail_psi_closed ? 1.0 : 2.0) * spin;
        // ... with the overlap matrix made early by the resident body (psi^H B times the Taylor sum: four tiles over the
        // ceil(M / 4) k-steps, two real multiplications each) in place of the tail's own
        if (p.early) out.closed += 2048.0 * (4.0 * ((M + 3) / 4) * 2.0 - t16 * t16 * ks1 * 2.0);
        out.total = out.open * f.nw;
    }
    return out;
}
