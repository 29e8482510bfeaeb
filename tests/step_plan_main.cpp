// The launch plan of the fused propagator (pauxy_amd/csrc/step_plan.h) on the host alone: reads one case per line,
//   M na nb nw order same_b b_real closed_form fusion scope overlap handover plain psi_real psi_closed operands tail_lds steps
// followed by `steps` flags (1: the step is announced), walks the steps as afq_propagate does -- does the step fuse; the
// launch with or without the tail; the hand-over the launch leaves for the next one -- and prints each launch's plan and
// plan_issued_flops.  tests/test_step_plan_cpu.py holds the output to what the library launched and counted on the device.
#include <cstdio>
#include "../pauxy_amd/csrc/step_plan.h"

int main() {
    StepFacts f;
    int same_b, b_real, overlap, handover, plain, psi_real, psi_closed, operands, steps;
    unsigned long tail_lds;
    while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %lu %d", &f.M, &f.na, &f.nb, &f.nw, &f.order, &same_b,
                      &b_real, &f.closed_mode, &f.fusion_mode, &f.fusion_scope, &overlap, &handover, &plain, &psi_real,
                      &psi_closed, &operands, &tail_lds, &steps) == 18) {
        f.same_b = same_b; f.b_real = b_real; f.tail_overlap = overlap; f.handover = handover; f.plain_step = plain;
        f.one_call = true;                          // (afq_propagate: begin and finish in one call)
        f.B2_ready = operands;
        f.handover_current = false;
        for (int k = 0; k < steps; ++k) {
            int announced;
            if (std::scanf("%d", &announced) != 1) return 2;
            f.announced = announced;
            f.tail = false;
            f.tail = step_plan(f).fuses;            // (no tail among the facts: whether the step fuses does not read it)
            f.mul3 = f.fusion_mode == 2;
            f.tail_lds = tail_lds; f.tail_psi_real = psi_real; f.tail_psi_closed = psi_closed;
            f.tail_shared_psi = true; f.tail_spin_sum = true; f.psiB_ready = operands;
            const StepPlan p = step_plan(f);
            const StepFlops n = plan_issued_flops(p);
            std::printf("%s|%.17g %.17g %.17g|supported %d resident_class %d fusion_shape %d narrow %d full %d rem4 %d hyb %d "
                        "contig %d symcols %d closed_try %d resident %d tail %d early %d consumes %d produces %d lds %zu%s\n",
                        p.supported ? step_variant_name(p.variant) : "", n.open, n.closed, n.total, p.supported,
                        p.resident_class, p.fusion_shape, p.narrow, p.full, p.rem4, p.hyb, p.contig, p.symcols, p.closed_try,
                        p.resident, (int)p.tail, p.early, p.consumes, p.produces, p.lds, p.refusal ? " REFUSED" : "");
            f.handover_current = p.produces;        // (nothing comes between two steps here)
        }
    }
    return 0;
}
