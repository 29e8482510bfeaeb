// The fused step's state on the handle (afq_handle::step): its switches, the host-made operands with what they were made
// of, the hand-over buffers with their validity, the transients of one step and the counts of the last launch.  What a launch
// is, given this state, is decided by step_plan.h; nothing outside this header writes a switch or a provenance pointer.
#pragma once
#include "greens_cache.h"
#include "step_plan.h"

// Whether the hand-over buffers (t0_next, t0_ready) describe the walkers as they are now.  A launch of the fused propagator
// that produced sets `current`; everything that writes phi, moves a walker to another slot, changes the propagator, the
// trial, the Taylor order or a switch of the step drops it, and so does every propagator launch that is not that kernel with
// the early overlap (k_prop_fused drops on entry and sets again behind a launch that produced).  A device pointer to phi
// handed out (afq_walkers_device_ptr) turns it off for the life of the handle: the caller may write through it.
struct StepHandover {
    bool current = false;
    bool enabled = true;
    void drop() { current = false; }
    void produced() { current = enabled; }
};

struct StepState {
    // ---- the switches.  FUSION: 0 never, 1 tail behind the 4-multiplication body, 2 behind the 3-multiplication one;
    // SCOPE: 0 announced one-call steps, 1 every step of the shape class; TAIL_OVERLAP: the mode-2 tail's overlap matrix
    // and inverse under the closing pass; HANDOVER: that launch also makes the next step's opening one-body pass;
    // CLOSED_FORM: 0 auto, 1 streamed deal, 2 V resident in registers (where eligible)
    enum Switch { FUSION = 0, SCOPE, TAIL_OVERLAP, HANDOVER, CLOSED_FORM, N_SWITCHES };
    static int largest(Switch s) { return s == FUSION || s == CLOSED_FORM ? 2 : 1; }
    // the one setter (afq_set_step_*, afq_set_propagator_closed_form): a value the switch does not have is refused before
    // anything is written; a change of any switch drops the hand-over
    bool set(Switch s, int value) {
        if (value < 0 || value > largest(s)) return false;
        sw[s] = value;
        handover.drop();
        return true;
    }
    int get(Switch s) const { return sw[s]; }

    // ---- the host-made operands (device blocks of the trial's lifetime; made by step_operands, afq_api.hip, whenever the
    // trial or the propagator is uploaded; null unless the trial is single, real and closed and BH1 real and the same for
    // both spins) and the device trial and propagator each was made of (compared, never dereferenced)
    double *psiB_cT = nullptr;      // psi^H B for the early overlap (k_fused_closed.h): [na, M], psiB_cT[i][k] = sum_m psi[m][i] BH1[0][m][k]
    double *B2 = nullptr;           // Re(BH1[0]) . Re(BH1[0]) for the step hand-over: [M, M], extended accumulation, one rounding
    void operands_gone() { psiB_psi = psiB_bh1 = b2_bh1 = nullptr; handover.drop(); }
    void made_psiB(const void *psi, const void *bh1) { psiB_psi = psi; psiB_bh1 = bh1; }
    void made_B2(const void *bh1) { b2_bh1 = bh1; }
    bool psiB_ready(const void *psi, const void *bh1) const { return psiB_cT && psi == psiB_psi && bh1 == psiB_bh1; }
    bool B2_ready(const void *bh1) const { return B2 && bh1 == b2_bh1; }

    // ---- the step hand-over of the 3-multiplication tail kernel: t0_next[w] holds T_0 = B phi[w] of the NEXT step as the
    // resident body's image of T, t0_ready[w] says for which walkers (written by every launch of that kernel); both are
    // allocated the first time a launch can produce (walkers' lifetime).  `handover` says whether they are about the CURRENT phi.
    unsigned char *t0_next = nullptr;   // [nw][ceil(M / 4) * 2048 B]
    int *t0_ready = nullptr;            // [nw]
    StepHandover handover;
    bool handover_current() const { return handover.current && t0_next && t0_ready; }

    // ---- one step.  afq_propagate (begin and finish in one call): the energy shift is known while the propagator is launched,
    // which may then take the step's closing Green's function along as its tail; tail_done tells the finish half that it has,
    // with what result
    bool one_call = false, tail_done = false;
    double2 eshift = {0.0, 0.0};
    GreensResult tail_res;
    bool vhs_upper = false;         // set around build_vhs + k_prop_fused: VHS[w] holds only its upper triangle

    // ---- matrix-pipe flops of the last fused-propagator launch (plan_issued_flops; afq_propagator_issued_flops)
    StepFlops issued;

private:
    int sw[N_SWITCHES] = {2, 0, 1, 1, 0};
    const void *psiB_psi = nullptr, *psiB_bh1 = nullptr, *b2_bh1 = nullptr;
};
