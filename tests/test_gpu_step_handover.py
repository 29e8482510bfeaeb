"""The step hand-over of the fused propagator's 3-multiplication tail kernel (afq_set_step_handover, k_fused_closed.h): under
the inversion of the tail's overlap matrix the idle waves of a resident walker make the opening one-body pass of the NEXT
step, T_0 = (B B) S, and the next launch starts that walker at its Taylor products -- unless the handle has dropped the
hand-over because something came between the two launches.

Shapes, population, fields, oracle and tolerances are tests.test_gpu_tail_overlap's: (M, n) = (97, 17), (100, 25), (104, 32),
K = 8, 33 walkers of which one is open-shell and one has weight zero, order 1, 3 and 6, scope 1, mode 2; 1e-10 per step taken
relative to the largest element against the oracle, twice that between two device forms.  Five steps: announced,
unannounced, split begin / finish, announced, announced.  Each (shape, order, mode, switch) runs once and is shared by the
tests below, unchanged."""
import ctypes
import functools

import numpy
import pytest

from oracle import afqmc_ref as ref
from pauxy_amd import _lib as L
from tests.test_gpu_pair_branch import DeviceBuffer
from tests.test_gpu_step_fusion import ESHIFT, launches, same_bits
from tests.test_gpu_sizes import close
from tests.test_gpu_tail_overlap import (DEAD, NW, OPEN, ORDERS, SHAPES, TOL, WALKER_FIELDS, check_against, one_step,
                                          oracle_steps, population, start)

KINDS = ('announced', 'unannounced', 'split', 'announced', 'announced')
LIVE_CLOSED = NW - 2
STATE = (L.F_PHI, L.F_WEIGHT, L.F_OT, L.F_HYBRID_ENERGY)


def handed(dev):
    return int(dev.counters(n=10)[9])


def step(dev, how):
    out = one_step(dev, how)
    out['handed'] = handed(dev)
    return out


@functools.lru_cache(maxsize=None)
def oracle(M, N, order):
    case = population(M, N, order)
    walkers = [ref.new_walker(case['model'], case['phis'][i]) for i in range(NW)]
    return oracle_steps(case['model'], walkers, case['w0'] != 0.0, 0, len(KINDS))


def run_once(M, N, order, mode, on):
    dev = start(population(M, N, order), mode, 1)
    try:
        dev.set_step_handover(on)
        dev.counters(reset=True, n=10)
        return [step(dev, how) for how in KINDS]
    finally:
        dev.close()


run = functools.lru_cache(maxsize=None)(run_once)


def walkers_from(model, state):
    """Oracle walkers in the state read back from the device."""
    walkers = []
    for i in range(NW):
        w = ref.new_walker(model, state[L.F_PHI][i], weight=float(state[L.F_WEIGHT][i]))
        w['ot'] = w['ovlp'] = complex(state[L.F_OT][i])
        w['hybrid_energy'] = complex(state[L.F_HYBRID_ENERGY][i])
        walkers.append(w)
    return walkers


def check_live(s, want, live, tol):
    for i in range(NW):
        if not live[i]:
            continue
        for f, key in ((L.F_PHI, 'phi'), (L.F_WEIGHT, 'weight'), (L.F_OT, 'ot'), (L.F_HYBRID_ENERGY, 'ehyb'), (L.F_XBAR, 'xbar')):
            close(s['fields'][f][i], want[key][i], tol)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_five_steps_against_the_oracle_and_the_switch_off(M, N, order):
    """phi, weight, overlap, hybrid energy and the next step's force bias (and the per-spin Ghalf of the unannounced step) on
    each of the five steps: against the oracle at TOL per step taken, against the same run with the switch off at twice
    that."""
    case, want = population(M, N, order), oracle(M, N, order)
    on, off = run(M, N, order, 2, 1), run(M, N, order, 2, 0)
    for k, (a, b) in enumerate(zip(on, off)):
        check_against(a, want[k], case, TOL * (k + 1), N)
        check_against(b, want[k], case, TOL * (k + 1), N)
        for f in WALKER_FIELDS:
            close(a['fields'][f], b['fields'][f], 2.0 * TOL * (k + 1))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_the_path_is_taken_and_nothing_else_is_counted_differently(M, N, order):
    """Counter [9]: nothing to start from on the first step, every live closed walker on each later one -- never the open-shell
    or the zero-weight walker.  The closed-deal, one-spin and early-overlap counters and the launches are the switch-off run's."""
    on, off = run(M, N, order, 2, 1), run(M, N, order, 2, 0)
    assert [s['handed'] for s in on] == [LIVE_CLOSED * k for k in range(len(KINDS))]
    assert [s['handed'] for s in off] == [0] * len(KINDS)
    for a, b in zip(on, off):
        assert (a['closed_prop'], a['closed_greens'], a['early']) == (b['closed_prop'], b['closed_greens'], b['early'])
        assert {n: c for n, (c, _ms) in a['trace'].items()} == {n: c for n, (c, _ms) in b['trace'].items()}
        assert launches(a['trace'], 'prop_fused_kernel<false, 7, true, true>') == 1


DROPS = ('reortho', 'copy', 'pack_unpack', 'upload_phi', 'set_propagator', 'closed_form', 'step_fusion', 'fusion_scope',
         'tail_overlap', 'handover')


@pytest.mark.gpu
@pytest.mark.parametrize("what", DROPS)
def test_whatever_comes_between_two_steps_drops_the_hand_over(what):
    """Two steps (the second consumes), one event, two more steps.  The step behind the event starts from phi -- counter [9]
    stands still -- and meets the oracle of the state read back behind the event (for the copy: walker 2's propagation in slot
    3; for the second BH1: the new propagator's); the step after consumes again.  A writer that forgot to drop would hand the
    step a T_0 of another phi, slot or propagator: an error of order one, not of rounding."""
    M, N = SHAPES[1]
    case, other = population(M, N, 6), population(M, N, 6, dt=0.005)
    model = case['model']
    live = case['w0'] != 0.0
    dev = start(case, 2, 1)
    try:
        dev.counters(reset=True, n=10)
        step(dev, 'announced')
        assert step(dev, 'announced')['handed'] == LIVE_CLOSED
        if what == 'reortho':
            dev.reortho()
        elif what == 'copy':
            dev.copy_walker(2, 3)
        elif what == 'pack_unpack':
            buf = DeviceBuffer(dev, dev.pack_bytes())
            dev.pack(2, buf.ptr.value)
            dev.unpack(3, buf.ptr.value)
            dev.sync()
        elif what == 'upload_phi':
            phi = dev.get(L.F_PHI)
            phi[5], phi[6] = phi[6].copy(), phi[5].copy()
            ot = dev.get(L.F_OT)
            ot[5], ot[6] = ot[6], ot[5]
            dev.set(L.F_PHI, phi)
            dev.set(L.F_OT, ot)
        elif what == 'set_propagator':
            model = other['model']
            assert not numpy.array_equal(case['model'].BH1, model.BH1)
            dev.set_propagator(model.BH1, model.mf_shift, model.dt, exp_order=6)
        elif what == 'closed_form':
            dev.set_propagator_closed_form(1)
            dev.set_propagator_closed_form(0)
        elif what == 'step_fusion':
            dev.set_step_fusion(0)
            dev.set_step_fusion(2)
        elif what == 'fusion_scope':
            dev.set_step_fusion_scope(0)
            dev.set_step_fusion_scope(1)
        elif what == 'tail_overlap':
            dev.set_step_tail_overlap(0)
            dev.set_step_tail_overlap(1)
        else:
            dev.set_step_handover(0)
            dev.set_step_handover(1)
        state = {f: dev.get(f) for f in STATE}
        if what == 'copy' or what == 'pack_unpack':
            assert same_bits(state[L.F_PHI][3], state[L.F_PHI][2])
        want = oracle_steps(model, walkers_from(model, state), live, 2, 2)
        s = step(dev, 'announced')
        assert s['handed'] == LIVE_CLOSED, what
        check_live(s, want[0], live, TOL)
        s = step(dev, 'announced')
        assert s['handed'] == 2 * LIVE_CLOSED, what
        check_live(s, want[1], live, 2.0 * TOL)
    finally:
        dev.close()


@pytest.mark.gpu
def test_a_walker_that_was_dead_for_a_step_starts_from_phi():
    """Walker 7's weight is 0 for the third step and 1 again for the fourth.  The launch that skipped it has cleared its flag:
    on the fourth step it runs the ordinary prologue although its phi never changed and the host holds the hand-over current,
    and meets the oracle; on the fifth it consumes again."""
    M, N = SHAPES[1]
    case = population(M, N, 6)
    model, live = case['model'], case['w0'] != 0.0
    dev = start(case, 2, 1)
    try:
        dev.counters(reset=True, n=10)
        step(dev, 'announced')
        assert step(dev, 'announced')['handed'] == LIVE_CLOSED
        weight = dev.get(L.F_WEIGHT)
        kept, weight[7] = weight[7], 0.0
        dev.set(L.F_WEIGHT, weight)
        before = dev.get(L.F_PHI)[7]
        s = step(dev, 'announced')
        assert s['handed'] == 2 * LIVE_CLOSED - 1 and same_bits(s['fields'][L.F_PHI][7], before)
        weight = dev.get(L.F_WEIGHT)
        assert weight[7] == 0.0
        weight[7] = kept
        dev.set(L.F_WEIGHT, weight)
        state = {f: dev.get(f) for f in STATE}
        want = oracle_steps(model, walkers_from(model, state), live, 3, 2)
        s = step(dev, 'announced')
        assert s['handed'] == 3 * LIVE_CLOSED - 2
        check_live(s, want[0], live, TOL)
        s = step(dev, 'announced')
        assert s['handed'] == 4 * LIVE_CLOSED - 2
        check_live(s, want[1], live, 2.0 * TOL)
    finally:
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("M,N", SHAPES)
def test_walkers_and_modes_outside_the_path_keep_every_bit(M, N):
    """The open-shell and the zero-weight walker: every field on every step is the switch-off run's, bit for bit.  Mode 1 (the
    4-multiplication tail) with the switch on gives mode 0's bits and never counts."""
    on, off = run(M, N, 6, 2, 1), run(M, N, 6, 2, 0)
    for k, (a, b) in enumerate(zip(on, off)):
        for f in WALKER_FIELDS:
            for i in (OPEN, DEAD):
                assert same_bits(a['fields'][f][i], b['fields'][f][i]), (k, f, i)
    for i in (OPEN, DEAD):
        assert same_bits(on[1]['ghalf'][i], off[1]['ghalf'][i])
    one, two = run(M, N, 6, 1, 1), run(M, N, 6, 0, 1)
    for k, (a, b) in enumerate(zip(one, two)):
        assert a['handed'] == 0 and b['handed'] == 0
        for f in WALKER_FIELDS:
            assert same_bits(a['fields'][f], b['fields'][f]), (k, f)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_a_second_handle_repeats_every_bit(M, N, order):
    first, again = run(M, N, order, 2, 1), run_once(M, N, order, 2, 1)
    for k, (a, b) in enumerate(zip(first, again)):
        assert a['handed'] == b['handed']
        for f in WALKER_FIELDS:
            assert same_bits(a['fields'][f], b['fields'][f]), (k, f)
    assert same_bits(first[1]['ghalf'], again[1]['ghalf'])


def test_switch_rejects_bad_values_and_null_handle():
    """No GPU: afq_set_step_handover takes 0 and 1 and nothing else, and refuses a null handle (a zeroed block stands in for
    the handle, which is only touched after the value check)."""
    lib = L.load()
    assert lib.afq_set_step_handover(None, 0) == L.AFQ_EINVAL
    assert lib.afq_set_step_handover(None, 1) == L.AFQ_EINVAL
    block = ctypes.create_string_buffer(1 << 16)
    h = ctypes.cast(block, L._h)
    for bad in (-1, 2, 3, 1 << 20):
        assert lib.afq_set_step_handover(h, bad) == L.AFQ_EINVAL, bad
    assert block.raw == bytes(1 << 16)
