"""Every public call between two steps, on warm caches, against the oracle: the table of tests/between_steps_cases.py on the
device.  One test per (configuration, warm state, event): reach the warm state, read the pure walker fields back, run the
event, read back again, and hold the announced step, the unannounced step, get(F_GHALF) and local_energy() behind it to the
oracle of the read-back state -- a handle that never cached anything.  A missed invalidation hands a walker another
walker's T_0, another phi's force bias or one spin's exchange energy: errors of order one, which the teeth of each row
(the event moved its operand by more than 1e-3 of its largest element) keep from hiding under the tolerance.

Tolerances are those of the tests that already hold each path: test_gpu_tail_overlap.TOL = 1e-10 per step taken behind the
read-back, relative to the largest element (test_gpu_sizes.close), for rhf64, rhf24, msd2, tail and ueg; for hub8x8 the
pair of test_blocked_gauss_jordan_hands_badly_placed_pivots_to_the_step_by_step_kernel, 1e-9 of the determinant for the
overlap and 1e-8 for Ghalf and what is made of it (phi, weight, hybrid energy, force bias); test_gpu_sizes.TOL for energies.
Walkers that are dead in the read-back state keep every bit through both steps.

On `tail` counter [9] (walker steps that started from a hand-over; its value behind the event is the baseline, since a row
may reset the counters) says the cache was warm: it stands still on the step
behind a row that writes phi, moves a walker or changes the propagator, trial or a step switch; it advances by the walkers
that are live and closed on both sides of a row that does neither (readers, and the weight / overlap / Ghalf uploads and
switches that touch nothing the hand-over is made of); it advances again on the second step, except behind rows that turn the
path off for the life of the handle (a device pointer handed out, a complex trial).

Shared: configurations and their oracle populations are cached (between_steps_cases.configuration)."""
import numpy
import pytest

from pauxy_amd import _lib as L
from tests import between_steps_cases as bs
from tests.test_gpu_sizes import TOL as ENERGY_TOL, close
from tests.test_gpu_tail_overlap import TOL

pytestmark = pytest.mark.gpu

CASES = bs.cases()
PAIRS = ((L.F_PHI, 'phi'), (L.F_WEIGHT, 'weight'), (L.F_OT, 'ot'), (L.F_HYBRID_ENERGY, 'ehyb'), (L.F_PHASE, 'phase'),
         (L.F_XBAR, 'xbar'))


def make(model, nw):
    from tests.helpers import make_device
    return make_device(model, nw)


def tolerances(config, k):
    """-> (overlap: relative to the determinant itself or None, everything else: relative to the largest element)"""
    if config == 'hub8x8':
        return 1e-9, 1e-8
    return None, TOL * k


def check_values(config, out):
    after, model = out['after'], out['model']
    nw = len(after[L.F_WEIGHT])
    live0 = bs.is_live(after[L.F_WEIGHT])
    for k, (got, want) in enumerate(out['steps'], 1):
        det_tol, tol = tolerances(config, k)
        for i in range(nw):
            if not live0[i]:
                for f in (L.F_PHI, L.F_WEIGHT, L.F_OT, L.F_HYBRID_ENERGY, L.F_PHASE):
                    assert bs.same_bits(got[f][i], after[f][i]), (k, i, f)
                continue
            for f, key in PAIRS:
                if want[key][i] is None:                   # (no force bias for a walker the step before has killed)
                    continue
                if f == L.F_OT and det_tol is not None:
                    assert abs(got[f][i] - want[key][i]) <= det_tol * abs(want[key][i]), (k, i, got[f][i], want[key][i])
                    continue
                try:
                    close(got[f][i], want[key][i], tol)
                except AssertionError as e:
                    raise AssertionError("step %d walker %d %s: %s" % (k, i, key, e))
    det_tol, tol = tolerances(config, 2)
    nt = model.na + model.nb
    last = out['steps'][-1][1]
    for i in range(nw):
        if not (live0[i] and bs.is_live(last['weight'][i])):
            continue
        try:
            close(out['ghalf'][i].reshape(nt, -1), out['want_ghalf'][i], tol)
            close(out['energy'][i], out['want_energy'][i], ENERGY_TOL)
        except AssertionError as e:
            raise AssertionError("behind the second step, walker %d: %s" % (i, e))


def check_hand_over(r, out):
    before, after, model = out['before'], out['after'], out['model']
    nw = len(after[L.F_WEIGHT])
    closed = numpy.array([bs.is_closed(after[L.F_PHI][i], model.na, model.nb) for i in range(nw)])
    same = numpy.array([bs.same_bits(after[L.F_PHI][i], before[L.F_PHI][i]) for i in range(nw)])
    live_b, live_a = bs.is_live(before[L.F_WEIGHT]), bs.is_live(after[L.F_WEIGHT])
    first, second = out['steps'][0][1], out['steps'][1][1]
    live_1 = numpy.array(first['live']) & numpy.array(second['live'])
    h0, h1, h2 = out['handed']
    assert out['warm_handed'] > 0, 'the second step of the warm-up consumed no hand-over'
    if r.hands == 'off':
        assert (h1 - h0, h2 - h1) == (0, 0), out['handed']
        return
    took = int((closed & same & live_b & live_a).sum()) if r.hands == 'on' else 0
    assert h1 - h0 == took, (r.name, out['handed'], took)
    assert h2 - h1 == int((closed & live_1).sum()), (r.name, out['handed'])
    assert took > 0 or r.hands == 'still'


@pytest.mark.parametrize("config,warm,name", CASES, ids=["%s-%s-%s" % c for c in CASES])
def test_the_steps_behind_an_event_are_those_of_a_handle_that_cached_nothing(config, warm, name):
    r = bs.ROW[name]
    out = bs.run_case(config, warm, name, make)
    bs.check_teeth(r, out)
    check_values(config, out)
    if config == 'tail' and r.hands is not None:
        check_hand_over(r, out)
