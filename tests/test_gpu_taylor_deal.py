"""The split deal of the resident closed-shell body's Taylor products (k_fused_closed.h, the 3-multiplication tail kernel):
slot 1 of row tiles 4-6 is cut along k at k-step KH = (KS + 1) / 2, the owner multiplies the lower k-steps, wave 7 the upper
ones of all three, and the owner adds wave 7's partial to its own ahead of the division by n.

Shapes, population, fields, oracle and tolerances are tests.test_gpu_tail_overlap's: (M, n) = (97, 17), (100, 25), (104, 32) --
KS = 25 with one live row in row tile 6, KS = 25, and KS = 26 with a 13 / 13 split -- K = 8, 33 walkers of which one is
open-shell and one has weight zero, order 1, 3 and 6 (the Taylor sum ends in either image of T), scope 1; an announced step,
an unannounced one, a split one, an announced one; 1e-10 per step taken relative to the largest element against the oracle
(tests.test_gpu_sizes.close).  Mode 2 with the tail overlap and the step hand-over each on and off.  Each (shape, order, mode,
switches) runs once and is shared by the tests below, unchanged.

Precision (test_a_k_sum_in_two_pieces_costs_one_rounding): the distance of one step's phi from a numpy.longdouble restatement
of B (sum V^n / n!) B phi, against the same distance measured with the build before the split deal on the same inputs
(profiles/taylor_deal_precision.md holds both columns): at most twice that."""
import functools

import numpy
import pytest

from oracle import afqmc_ref as ref
from pauxy_amd import _lib as L
from tests.philox_ref import device_normals_fast
from tests.test_gpu_step_fusion import SEED, launches, same_bits
from tests.test_gpu_tail_overlap import (DEAD, K, KINDS, NW, OPEN, ORDERS, SHAPES, TOL, WALKER_FIELDS, check_against,
                                         clipped_force_bias, one_step, oracle, population, start)

LIVE_CLOSED = NW - 2
SWITCHES = [(1, 1), (1, 0), (0, 0)]         # (tail overlap, step hand-over): the hand-over exists under the overlap alone

# dev.propagator_issued_flops() = (open, closed) per walker behind each of the four steps, recorded from the build before the
# split deal: {(M, n, order, overlap, hand-over): ((open, closed) x 4)}.  The deal issues not one MFMA more or fewer.
ISSUED = {
    (97, 17, 1, 1, 1): ((11096064.0, 7290880.0), (11096064.0, 5857280.0), (11096064.0, 5857280.0), (11096064.0, 5857280.0)),
    (97, 17, 1, 1, 0): ((11096064.0, 5857280.0), (11096064.0, 5857280.0), (11096064.0, 5857280.0), (11096064.0, 5857280.0)),
    (97, 17, 1, 0, 0): ((11096064.0, 5906432.0), (11096064.0, 5906432.0), (11096064.0, 5906432.0), (11096064.0, 5906432.0)),
    (97, 17, 3, 1, 1): ((19083264.0, 11591680.0), (19083264.0, 10158080.0), (19083264.0, 10158080.0), (19083264.0, 10158080.0)),
    (97, 17, 3, 1, 0): ((19083264.0, 10158080.0), (19083264.0, 10158080.0), (19083264.0, 10158080.0), (19083264.0, 10158080.0)),
    (97, 17, 3, 0, 0): ((19083264.0, 10207232.0), (19083264.0, 10207232.0), (19083264.0, 10207232.0), (19083264.0, 10207232.0)),
    (97, 17, 6, 1, 1): ((31064064.0, 18042880.0), (31064064.0, 16609280.0), (31064064.0, 16609280.0), (31064064.0, 16609280.0)),
    (97, 17, 6, 1, 0): ((31064064.0, 16609280.0), (31064064.0, 16609280.0), (31064064.0, 16609280.0), (31064064.0, 16609280.0)),
    (97, 17, 6, 0, 0): ((31064064.0, 16658432.0), (31064064.0, 16658432.0), (31064064.0, 16658432.0), (31064064.0, 16658432.0)),
    (100, 25, 1, 1, 1): ((10721280.0, 7462912.0), (10721280.0, 6029312.0), (10721280.0, 6029312.0), (10721280.0, 6029312.0)),
    (100, 25, 1, 1, 0): ((10721280.0, 6029312.0), (10721280.0, 6029312.0), (10721280.0, 6029312.0), (10721280.0, 6029312.0)),
    (100, 25, 1, 0, 0): ((10721280.0, 6078464.0), (10721280.0, 6078464.0), (10721280.0, 6078464.0), (10721280.0, 6078464.0)),
    (100, 25, 3, 1, 1): ((17270784.0, 11763712.0), (17270784.0, 10330112.0), (17270784.0, 10330112.0), (17270784.0, 10330112.0)),
    (100, 25, 3, 1, 0): ((17270784.0, 10330112.0), (17270784.0, 10330112.0), (17270784.0, 10330112.0), (17270784.0, 10330112.0)),
    (100, 25, 3, 0, 0): ((17270784.0, 10379264.0), (17270784.0, 10379264.0), (17270784.0, 10379264.0), (17270784.0, 10379264.0)),
    (100, 25, 6, 1, 1): ((27095040.0, 18214912.0), (27095040.0, 16781312.0), (27095040.0, 16781312.0), (27095040.0, 16781312.0)),
    (100, 25, 6, 1, 0): ((27095040.0, 16781312.0), (27095040.0, 16781312.0), (27095040.0, 16781312.0), (27095040.0, 16781312.0)),
    (100, 25, 6, 0, 0): ((27095040.0, 16830464.0), (27095040.0, 16830464.0), (27095040.0, 16830464.0), (27095040.0, 16830464.0)),
    (104, 32, 1, 1, 1): ((12730368.0, 7823360.0), (12730368.0, 6332416.0), (12730368.0, 6332416.0), (12730368.0, 6332416.0)),
    (104, 32, 1, 1, 0): ((12730368.0, 6332416.0), (12730368.0, 6332416.0), (12730368.0, 6332416.0), (12730368.0, 6332416.0)),
    (104, 32, 1, 0, 0): ((12730368.0, 6365184.0), (12730368.0, 6365184.0), (12730368.0, 6365184.0), (12730368.0, 6365184.0)),
    (104, 32, 3, 1, 1): ((21676032.0, 12296192.0), (21676032.0, 10805248.0), (21676032.0, 10805248.0), (21676032.0, 10805248.0)),
    (104, 32, 3, 1, 0): ((21676032.0, 10805248.0), (21676032.0, 10805248.0), (21676032.0, 10805248.0), (21676032.0, 10805248.0)),
    (104, 32, 3, 0, 0): ((21676032.0, 10838016.0), (21676032.0, 10838016.0), (21676032.0, 10838016.0), (21676032.0, 10838016.0)),
    (104, 32, 6, 1, 1): ((35094528.0, 19005440.0), (35094528.0, 17514496.0), (35094528.0, 17514496.0), (35094528.0, 17514496.0)),
    (104, 32, 6, 1, 0): ((35094528.0, 17514496.0), (35094528.0, 17514496.0), (35094528.0, 17514496.0), (35094528.0, 17514496.0)),
    (104, 32, 6, 0, 0): ((35094528.0, 17547264.0), (35094528.0, 17547264.0), (35094528.0, 17547264.0), (35094528.0, 17547264.0)),
}

# max |phi - phi_longdouble| / max |phi_longdouble| over the closed walkers of one announced step, order 6, mode 2 with both
# switches on, measured with the build before the split deal (profiles/taylor_deal_precision.md)
PARENT_DISTANCE = {
    (97, 17): 1.8424015586558266e-15,
    (100, 25): 1.7417830623250947e-15,
    (104, 32): 2.2835710158205037e-15,
}


def run_once(M, N, order, mode, on, ho):
    dev = start(population(M, N, order), mode, on)
    try:
        dev.set_step_handover(ho)
        dev.counters(reset=True, n=10)
        steps = []
        for how in KINDS:
            s = one_step(dev, how)
            s['handed'] = int(dev.counters(n=10)[9])
            s['issued'] = tuple(float(x) for x in dev.propagator_issued_flops())
            steps.append(s)
        return steps
    finally:
        dev.close()


run = functools.lru_cache(maxsize=None)(run_once)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("on,ho", SWITCHES)
def test_four_steps_against_the_oracle(M, N, order, on, ho):
    """phi, weight, overlap, hybrid energy and the force bias the next step made, on each step; the spin blocks of every
    closed walker bitwise equal and the open-shell walker's not (check_against); the path counters."""
    case, want = population(M, N, order), oracle(M, N, order)
    for k, s in enumerate(run(M, N, order, 2, on, ho)):
        check_against(s, want[k], case, TOL * (k + 1), N)
        phi = s['fields'][L.F_PHI]
        for i in range(NW):
            if i not in (OPEN, DEAD):
                assert same_bits(phi[i, :, :N], phi[i, :, N:]), (k, i)
        assert s['closed_prop'] == LIVE_CLOSED * (k + 1)
        assert s['early'] == (LIVE_CLOSED * (k + 1) if on else 0)
        assert s['handed'] == (LIVE_CLOSED * k if ho else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_open_and_dead_walkers_keep_the_bits_of_mode_1(M, N, order):
    """Neither takes the resident body: every field of both, on every step, is what the same build gives in mode 1 (the
    4-multiplication tail kernel, which the deal does not touch)."""
    one = run(M, N, order, 1, 1, 1)
    for on, ho in SWITCHES:
        for k, (a, b) in enumerate(zip(run(M, N, order, 2, on, ho), one)):
            for f in WALKER_FIELDS:
                for i in (OPEN, DEAD):
                    assert same_bits(a['fields'][f][i], b['fields'][f][i]), (on, ho, k, f, i)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_switches_move_no_bit_of_the_first_step(M, N, order):
    """Both 3-multiplication bodies deal and combine alike, and a walker that starts from phi makes the same T_0 with the
    hand-over on or off: the first step's phi and force bias are the same bits under every pair of switches."""
    first = [run(M, N, order, 2, on, ho)[0]['fields'] for on, ho in SWITCHES]
    for other in first[1:]:
        assert same_bits(first[0][L.F_PHI], other[L.F_PHI])
        assert same_bits(first[0][L.F_XBAR], other[L.F_XBAR])


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_a_second_handle_repeats_every_bit(M, N, order):
    """The owner adds wave 7's partial to its own in one fixed order: nothing depends on which wave arrives first."""
    for a, b in zip(run_once(M, N, order, 2, 1, 1), run(M, N, order, 2, 1, 1)):
        for f in WALKER_FIELDS:
            assert same_bits(a['fields'][f], b['fields'][f]), f
        if 'ghalf' in a:
            assert same_bits(a['ghalf'], b['ghalf'])


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("on,ho", SWITCHES)
def test_issued_flops_are_what_they_were(M, N, order, on, ho):
    assert tuple(s['issued'] for s in run(M, N, order, 2, on, ho)) == ISSUED[(M, N, order, on, ho)]


@pytest.mark.gpu
@pytest.mark.parametrize("on,ho", SWITCHES)
def test_a_step_launches_what_it_launched_before(on, ho):
    """What tests.test_gpu_tail_overlap pins: one propagator launch per step, the 3-multiplication tail kernel under its name; a
    Green's function launch only ahead of the first step; one weight_kernel on the split step and none elsewhere."""
    M, N = SHAPES[1]
    steps = run(M, N, 6, 2, on, ho)
    assert [launches(s['trace'], 'prop_fused_kernel') for s in steps] == [1, 1, 1, 1]
    assert [launches(s['trace'], 'prop_fused_kernel<false, 7, true, true>') for s in steps] == [1, 1, 1, 1]
    assert [launches(s['trace'], 'greens_small_kernel') for s in steps] == [1, 0, 0, 0]
    assert [launches(s['trace'], 'weight_kernel') for s in steps] == [0, 0, 1, 0]
    assert launches(steps[1]['ghalf_trace'], 'greens_small_kernel') == 0


def longdouble_step(model, phi, xi):
    """B (sum_{n <= order} V^n / n!) B phi on the alpha half in numpy.longdouble; V and the fields as the oracle makes them, in
    double (the step's inputs, the same for every build)."""
    N = model.na
    xbar = clipped_force_bias(model, phi)
    xs = ref.shift_fields(xi, xbar, model.mf_shift, model.sqrt_dt)[0]
    V = numpy.asarray(model.vhs(xs)).astype(numpy.clongdouble)
    B = numpy.asarray(model.BH1[0]).real.astype(numpy.longdouble)
    T = B @ phi[:, :N].astype(numpy.clongdouble)
    S = T.copy()
    for n in range(1, model.exp_order + 1):
        T = (V @ T) / numpy.longdouble(n)
        S = S + T
    return B @ S


def distance(M, N, got_phi):
    """max over the closed walkers of |phi - phi_longdouble| relative to the largest element, one step of order 6."""
    case = population(M, N, 6)
    xi = device_normals_fast(NW * K, SEED[0], SEED[1], 0).reshape(NW, K)
    worst = 0.0
    for i in range(NW):
        if i in (OPEN, DEAD):
            continue
        want = longdouble_step(case['model'], case['phis'][i], xi[i])
        worst = max(worst, float(numpy.abs(got_phi[i, :, :N] - want).max() / numpy.abs(want).max()))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("M,N", SHAPES)
def test_a_k_sum_in_two_pieces_costs_one_rounding(M, N):
    """A k sum in two pieces adds one rounding of the partial; anything beyond twice the distance of the build before is a
    defect of the combine."""
    d = distance(M, N, run(M, N, 6, 2, 1, 1)[0]['fields'][L.F_PHI])
    print("taylor deal precision (M, n) = (%d, %d): %.3e against %.3e before" % (M, N, d, PARENT_DISTANCE[(M, N)]))
    assert d <= 2.0 * PARENT_DISTANCE[(M, N)]
