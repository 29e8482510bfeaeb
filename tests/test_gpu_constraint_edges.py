"""The decision branches of the phaseless constraint on every path of the step: the force-bias bound (both copies of the
clipping, host fields, device Philox fields, the Hubbard variant that builds its site factors from the clipped field), both
sides of the hybrid / local-energy bound and the no-bound rule for eshift = 0, the phase kill, infinite and vanishing
importance functions, the weight cap behind a kill -- in each of the kernels the weight update is inlined into:
greens_tiny_kernel, greens_small_kernel, weight_kernel, det_combine_kernel here; the fifth, the fused propagator with the
Green's function as its tail (prop_fused_kernel<false, 7, true, MUL3>), never launches on the unannounced default-scope
steps taken here (the ``tail-*`` cases assert that, and run the two launches with the spin-sum force bias instead): the
routes to it are tests/test_gpu_constraint_tail.py's.

Two steps through the C ABI on the populations of tests/constraint_cases.py (checked on the reference alone in
tests/test_constraint_cases_cpu.py: no decision is closer than 1e-6 to its threshold), EVERY walker against the oracle
after each step: continuous values to 1e-9 (``close`` of tests/test_gpu_traj.py), decisions exactly -- the device counters,
weights of exactly 0, bounded energies on the bound, untouched walkers bit for bit.  Each case asserts the kernels it ran."""
import numpy
import pytest

from pauxy_amd import _lib as L
from tests import constraint_cases as cc
from tests.helpers import make_device
from tests.test_gpu_traj import close

pytestmark = pytest.mark.gpu
TOL = 1e-9
EST = [0, 1, 2, 3, 5, 6, 7, 8]        # uweight, weight, enumer, edenom, e1b, e2b, ehyb, ovlp (estimators/mixed.py:460-469)


def check_step(dev, model, eshift, extra, verdicts, before):
    """The device after a step against the oracle's verdicts; ``before``: the device's walkers ahead of the step."""
    hybrid = extra['hybrid']
    ebound = (2.0 / model.dt) ** 0.5
    got = {f: dev.get(f) for f in (L.F_PHI, L.F_WEIGHT, L.F_OT, L.F_HYBRID_ENERGY, L.F_ELOC, L.F_PHASE, L.F_XBAR,
                                   L.F_XSHIFTED)}
    counters = dev.counters(reset=True, n=8)
    live = [v for v in verdicts if v['live']]
    assert (int(counters[0]), int(counters[1])) == (sum(v['nfb'] for v in live), sum(v['nhe'] for v in live))
    for i, v in enumerate(verdicts):
        if not v['live']:
            # not propagated: bit-identical (a cap, where set, is above every parked weight)
            for f in (L.F_PHI, L.F_WEIGHT, L.F_OT, L.F_HYBRID_ENERGY, L.F_ELOC, L.F_PHASE):
                assert numpy.array_equal(got[f][i], before[f][i]), (i, f)
            continue
        close(got[L.F_XBAR][i], v['xbar'], TOL)
        close(got[L.F_XSHIFTED][i], v['xshifted'], TOL)
        assert numpy.array_equal(numpy.abs(got[L.F_XBAR][i]) > 1.0 - 1e-9, v['mask']), i
        assert numpy.max(numpy.abs(numpy.abs(got[L.F_XBAR][i][v['mask']]) - 1.0), initial=0.0) < 1e-14, i
        close(got[L.F_PHI][i], v['phi'], TOL)
        close(got[L.F_WEIGHT][i], v['weight'], TOL)
        close(got[L.F_OT][i], v['ot'], TOL)
        close(got[L.F_HYBRID_ENERGY][i], v['hybrid_energy'], TOL)
        close(got[L.F_ELOC][i], v['eloc'], TOL)
        close(got[L.F_PHASE][i], v['phase'], TOL)
        if v['weight'] == 0.0:
            assert got[L.F_WEIGHT][i] == 0.0, i
        else:
            assert got[L.F_WEIGHT][i] > 0.0, i
        if hybrid and v['side'] != 0:
            e = got[L.F_HYBRID_ENERGY][i]
            assert abs(e.real - (eshift + v['side'] * ebound)) <= 1e-13 * max(1.0, abs(eshift) + ebound), i
            close(e.imag, v['e_unbounded'].imag, TOL)
    return got, counters


def load_case(dev, run):
    """A fresh handle made ready for the first step of a case: walkers, weights, overlaps and energies as the oracle starts
    from them, the cap, the back-propagation window, the Philox seed; counters at zero."""
    model, phis, weights, xi, eshift, extra = run['case']
    if extra['msd_fb_mode']:
        dev.set_msd_force_bias(extra['msd_fb_mode'])
    dev.set(L.F_PHI, phis)
    dev.set(L.F_WEIGHT, weights)
    dev.set(L.F_UNSCALED_WEIGHT, weights)
    dev.set(L.F_OT, run['ot0'])
    dev.set(L.F_HYBRID_ENERGY, extra['ehyb0'])
    dev.set(L.F_ELOC, extra['ehyb0'])
    if extra['cap'] is not None:
        dev.set_weight_cap(*extra['cap'])
    if extra['bp']:
        dev.bp_configure(extra['bp'])
    if extra['philox'] is not None:
        dev.rng_seed(*extra['philox'])
    dev.counters(reset=True)


def check_bp_window(dev, run):
    """The back-propagation window the second step closed: the steps each walker recorded, then denominator and Green's
    function with the weights restored partially, against the oracle's."""
    model, weights = run['case'][0], run['case'][2]
    assert numpy.array_equal(dev.bp_steps(), run['bp_steps'])
    energies, denom, G = dev.bp_update(model.psi, 10, 'partial')
    want = run['bp_est']
    assert numpy.all(numpy.isfinite(G)) and numpy.isfinite(denom) and numpy.all(numpy.isfinite(energies))
    close(denom, want[3], TOL)
    close(G, want[4:].reshape(2, model.M, model.M), TOL)
    assert numpy.all(energies == 0)
    assert list(dev.bp_steps()) == [0] * len(weights)


def run_case(name, fusion=None):
    """``fusion``: (mode, scope) of afq_set_step_fusion / afq_set_step_fusion_scope, the handle's defaults when None."""
    run = cc.run_oracle(name)
    model, phis, weights, xi, eshift, extra = run['case']
    nw = len(weights)
    dev = make_device(model, nw, hybrid=extra['hybrid'])
    try:
        load_case(dev, run)
        if fusion is not None:
            dev.set_step_fusion(fusion[0])
            dev.set_step_fusion_scope(fusion[1])
        dev.launch_trace(True)
        state = {f: dev.get(f) for f in (L.F_PHI, L.F_WEIGHT, L.F_OT, L.F_HYBRID_ENERGY, L.F_ELOC, L.F_PHASE)}
        closed_steps = 0
        for x, verdicts in zip((xi, extra['xi2']), run['verdicts']):
            dev.propagate(None if extra['philox'] is not None else x, eshift)
            state, counters = check_step(dev, model, eshift, extra, verdicts, state)
            closed_steps += int(counters[3])
        launched = sorted(dev.launch_trace_get())
        dev.launch_trace(False)
        print("\n%s ran: %s" % (name, ", ".join(launched)))
        for k in extra['kernels']:
            assert any(k in n for n in launched), (k, launched)
        for k in extra['absent']:
            assert not any(k in n for n in launched), (k, launched)
        if extra['closed_deal']:
            assert closed_steps > 0                     # (the closed-shell deal of the fused propagator took them)
        # block estimates over what the second step left: the denominator and the weighted hybrid energy see the survivors
        dev.estimates_update(True)
        est = dev.estimates_get(zero=True)
        close(est[EST], run['estimates'][EST], TOL)
        if extra['bp']:
            check_bp_window(dev, run)
    finally:
        dev.close()


@pytest.mark.parametrize("name", cc.names())
def test_constraint_branches(name):
    run_case(name)


def test_standalone_field_kernel_clips():
    """afq_shift_fields: the field kernel without the fused force bias, every walker (it has no alive flags), on the
    unclipped force bias of a case with a mixed mask."""
    from oracle import afqmc_ref as ref
    run = cc.run_oracle('wgj-closed')
    model, phis, weights, xi, eshift, extra = run['case']
    first = run['verdicts'][0]
    nw, K = len(weights), model.nfields
    rng = numpy.random.RandomState(4)
    raw = numpy.array([v['xbar_raw'] if v['live'] else 0.7 * (rng.normal(size=K) + 1j * rng.normal(size=K)) for v in first])
    assert 0.1 < numpy.mean(numpy.abs(raw) > 1.0) < 0.9 and numpy.min(numpy.abs(numpy.abs(raw) - 1.0)) > cc.GUARD
    dev = make_device(model, nw)
    try:
        dev.launch_trace(True)
        xs, cmf, cfb = dev.shift_fields(xi, raw)
        assert any('fields_kernel<false>' in n for n in dev.launch_trace_get())
        for i in range(nw):
            want = ref.shift_fields(xi[i], raw[i], model.mf_shift, model.sqrt_dt)
            close(xs[i], want[0], TOL)
            close(cmf[i], want[1], TOL)
            close(cfb[i], want[2], TOL)
            clipped = numpy.abs(raw[i]) > 1.0
            assert numpy.max(numpy.abs(numpy.abs(xi[i] - xs[i])[clipped] - 1.0), initial=0.0) < 1e-14
    finally:
        dev.close()
