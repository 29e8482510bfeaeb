"""Fused propagator, closed-shell body with the HS potential resident in registers (k_fused_closed.h,
afq_set_propagator_closed_form): a population of closed, open and dead walkers, two steps against the oracle
(propagation/continuous.py:232-262), in the pattern of test_fused_propagator_closed_shell_deals.

The body exists for ONE REAL one-body matrix for both spins.  The builders' complex Cholesky vectors make BH1 complex (the
mean-field shift is), so for the complex L forms the eligible cases take the real part of that BH1 as the model's one-body
propagator -- device and oracle read the same arrays -- which sends the non-symmetric V of complex L (read in full, no
upper-triangle storage) through the body; the BH1 as built is the not-eligible case."""
import numpy
import pytest

from oracle import afqmc_ref as ref
from pauxy_amd import _lib as L
from tests.helpers import lform_params, make_device
from tests.test_gpu_sizes import assert_complex_rchol, build, close

pytestmark = pytest.mark.gpu
K, NW, STEPS = 24, 21, 2

_cases = {}


def population(M, N, lform, real_b=True, order=6):
    """Model, walkers, fields and the oracle's two steps for one case: computed once, shared by the tests, left unchanged."""
    key = (M, N, lform, real_b, order)
    if key in _cases:
        return _cases[key]
    model, rng = build(M, K, N, N, False, seed=31, lform=lform)
    assert_complex_rchol(model, lform)
    if real_b:
        model.BH1 = numpy.ascontiguousarray(model.BH1.real).astype(complex)
    model.exp_order = order
    assert numpy.array_equal(model.BH1[0], model.BH1[1])
    half = model.psi[None, :, :N] + 0.1 * (rng.rand(NW, M, N) + 1j * rng.rand(NW, M, N))
    phis = numpy.concatenate([half, half], axis=2)
    is_open = numpy.arange(NW) % 3 == 1
    phis[is_open, :, N:] += 0.05 * (rng.rand(int(is_open.sum()), M, N) + 1j * rng.rand(int(is_open.sum()), M, N))
    w0 = numpy.ones(NW)
    w0[4::7] = 0.0
    ot = numpy.array([ref.calc_overlap(p, model.psi, N, N) for p in phis])
    xis = [rng.normal(size=(NW, K)) for _ in range(STEPS)]
    walkers = [ref.new_walker(model, phis[i]) for i in range(NW)]
    want = []
    for step in range(STEPS):
        for i in range(NW):
            if w0[i] != 0.0:
                ref.propagate_walker_phaseless(model, walkers[i], xis[step][i], 0.2)
        want.append(([numpy.array(w['phi']) for w in walkers], [w['weight'] for w in walkers]))
    for a in (phis, w0, ot, is_open):
        a.setflags(write=False)
    _cases[key] = dict(model=model, phis=phis, is_open=is_open, w0=w0, ot=ot, xis=xis, want=want)
    return _cases[key]


def run(case, N, mode, form, counted):
    """Two steps on the device in `mode`; every walker of every step against the oracle, spin blocks, dead walkers and
    afq_counters [3].  form: what afq_propagator_closed_form must report; counted: a closed-shell deal exists at all."""
    model, phis, is_open, w0 = case['model'], case['phis'], case['is_open'], case['w0']
    dev = make_device(model, NW)
    dev.set_propagator_closed_form(mode)
    assert dev.propagator_closed_form() == form
    dev.set(L.F_PHI, phis)
    dev.set(L.F_WEIGHT, w0)
    dev.set(L.F_OT, case['ot'])
    dev.counters(reset=True)
    live_closed = int(((w0 > 0) & ~is_open).sum())
    outs = []
    for step in range(STEPS):
        dev.propagate(case['xis'][step], 0.2)
        out_phi, out_w = dev.get(L.F_PHI), dev.get(L.F_WEIGHT)
        want_phi, want_w = case['want'][step]
        for i in range(NW):
            if w0[i] == 0.0:
                assert numpy.array_equal(out_phi[i], phis[i]) and out_w[i] == 0.0
                continue
            close(out_phi[i], want_phi[i], 1e-10 * (step + 1))
            close(out_w[i], want_w[i], 1e-10 * (step + 1))
            assert numpy.array_equal(out_phi[i, :, :N], out_phi[i, :, N:]) == (not is_open[i]), (step, i)
        assert int(dev.counters()[3]) == (live_closed * (step + 1) if counted else 0)
        outs.append((out_phi, out_w))
    dev.close()
    return outs


ELIGIBLE = [(100, 25), (100, 17), (100, 32), (97, 20), (101, 32), (104, 20)]


@pytest.mark.parametrize("mode", [2, 0])
@pytest.mark.parametrize("M,N,lform", lform_params(ELIGIBLE, ['real', 'hermitian', 'general']))
def test_resident_body_eligible_shapes(M, N, lform, mode):
    """Both k-step counts (25: M <= 100, 26), the smallest and the largest electron count, row tile 6 with 1, 4, 5 and 8 live
    rows; symmetric V in upper-triangle storage (real L) and V read in full (complex L).  Forced (2) and automatic (0)."""
    run(population(M, N, lform), N, mode, 2, True)


@pytest.mark.parametrize("M,N,lform", lform_params([(100, 25), (104, 20)], ['real', 'general']))
def test_streamed_deal_against_resident_body(M, N, lform):
    """Mode 1 against mode 2 on the same inputs: both hold the oracle tolerance; their largest difference is reported."""
    case = population(M, N, lform)
    streamed = run(case, N, 1, 1, True)
    resident = run(case, N, 2, 2, True)
    for step in range(STEPS):
        diff = float(numpy.max(numpy.abs(streamed[step][0] - resident[step][0])))
        equal = numpy.array_equal(streamed[step][0], resident[step][0]) and numpy.array_equal(streamed[step][1], resident[step][1])
        print("M=%d N=%d %s step %d: max |phi(streamed) - phi(resident)| = %.3e, bit equal: %s" % (M, N, lform, step, diff, equal))


@pytest.mark.parametrize("M,N,lform,real_b,counted", [
    (96, 20, 'real', True, True),          # six row tiles: prop_fused_kernel<false, 6>, its own closed-shell deal
    (100, 16, 'real', True, False),        # one column tile per spin: no closed-shell deal at seven row tiles
    (100, 25, 'hermitian', False, True),   # complex BH1 (complex mean-field shift): the streamed deal
])
def test_resident_body_not_eligible(M, N, lform, real_b, counted):
    """Mode 2 outside the shape class takes the streamed path: correct results, the counter as before."""
    case = population(M, N, lform, real_b=real_b)
    if not real_b:
        assert numpy.abs(case['model'].BH1.imag).max() > 0.0
    run(case, N, 2, 1, counted)


def test_resident_body_taylor_order():
    """The order is a run-time loop around the unrolled product (and decides which LDS image the closing pass reads)."""
    run(population(100, 25, 'real', order=4), 25, 2, 2, True)
    run(population(100, 25, 'real', order=3), 25, 2, 2, True)
