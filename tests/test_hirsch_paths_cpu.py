"""The fixtures of tests/test_gpu_hirsch_paths.py, checked on the oracle alone (tests/hirsch_path_cases.py): every direct
case has a dead walker and one the first kinetic step kills, no uniform of a live walker is within 1e-6 of the probability
it is compared with, every ratio the direct update tests lies at least 0.2 rad inside pi / 2 -- but the one of the walker the
kill case names, which lies at least 0.2 rad beyond it and is the only one killed; the free-projection cases have a dead and
a parked walker that come back untouched; the back-propagation windows hold histories of different lengths that count.
Run with -s for the margins per case."""
import math

import numpy
import pytest

from tests import hirsch_path_cases as hc


@pytest.mark.parametrize("name", sorted(hc.DIRECT))
def test_direct_case_is_not_marginal(name):
    run = hc.run_direct(name)
    m, phis, w0, ot0, u = run['case']
    hc.check_direct(name, run)
    entered = ~numpy.isnan(run['arg'])
    print("\n%s: M=%d %d+%d nw=%d, %d walkers updated | min |u - pp/norm| %.1e | max |arg| of the passing ratios %.3f"
          % (name, m.M, m.na, m.nb, len(w0), entered.sum(), numpy.min(run['gap']),
             max([abs(a) for i, a in enumerate(run['arg']) if entered[i] and i != hc.DIRECT[name].get('kill')])))
    # dead and kinetic-killed walkers: nothing after the first call touches them
    assert numpy.array_equal(run['finish']['phi'][hc.DEAD], phis[hc.DEAD]) and run['finish']['ot'][hc.DEAD] == ot0[hc.DEAD]
    assert run['kinetic']['weight'][hc.FLIPPED] == 0.0 and run['kinetic']['ot'][hc.FLIPPED] == ot0[hc.FLIPPED]
    for k in ('phi', 'ot', 'weight'):
        assert numpy.array_equal(run['finish'][k][hc.FLIPPED], run['kinetic'][k][hc.FLIPPED])


def test_kill_case_kills_the_named_walker_only():
    """Im(gamma) (N_e - M) = -2.2 rad on 6 x 6 with 13 + 12 electrons: the walker whose sites all take field 0 is killed by the
    direct update whatever it looks like, its tracked overlap stays what the kinetic step left, the others pass."""
    name = '6x6-charge-kill'
    run = hc.run_direct(name)
    m = run['case'][0]
    k = hc.DIRECT[name]['kill']
    want = m.gamma.imag * (m.na + m.nb - m.M)
    assert abs(m.gamma.real) < 1e-15 and abs(run['arg'][k] - want) < 1e-9
    assert abs(run['arg'][k]) >= 0.5 * math.pi + hc.ARG_GUARD
    assert run['two_body']['weight'][k] == 0.0 and run['two_body']['ot'][k] == run['kinetic']['ot'][k]
    assert numpy.array_equal(run['finish']['phi'][k], run['two_body']['phi'][k])
    others = [i for i in range(len(run['arg'])) if i != k and not numpy.isnan(run['arg'][i])]
    assert len(others) >= 2 and all(run['two_body']['weight'][i] != 0.0 for i in others)
    assert all(abs(run['arg'][i]) <= 0.5 * math.pi - hc.ARG_GUARD for i in others)


@pytest.mark.parametrize("name", sorted(hc.FREE))
def test_free_case_skips_dead_and_parked_walkers(name):
    run = hc.run_free(name)
    m, phis, w0, ot0, u = run['case']
    assert w0[hc.DEAD] == 0.0 and w0[hc.PARKED] == 5e-9
    for s in run['steps']:
        for i in (hc.DEAD, hc.PARKED):
            assert numpy.array_equal(s['phi'][i], phis[i]) and s['weight'][i] == w0[i] and s['ot'][i] == ot0[i]
            assert s['phase'][i] == 1.0 and numpy.all(s['fields'][i] == -1)
        live = numpy.abs(w0) > 1e-8
        assert live.sum() >= 1 and numpy.all(s['fields'][live] >= 0) and numpy.all(s['weight'][live] > 1e-8)
    # only the charge decomposition's complex aux_wfac moves the phase
    moved = max(numpy.max(numpy.abs(s['phase'] - 1.0)) for s in run['steps'])
    assert moved > 1e-3 if hc.FREE[name]['charge'] else moved == 0.0, (name, moved)


@pytest.mark.parametrize("name", ['3x3-spin', '6x6-charge'])
def test_bp_case_holds_histories_of_different_lengths(name):
    """(The 64-walker window is checked where it is used: the oracle needs ten seconds for it.)"""
    run = hc.run_bp(name)
    spec = hc.BP[name]
    first, second = run['steps']
    assert first[hc.SRC] == first[hc.DST] == spec['nbp']
    assert 0 < first[hc.DEAD] == spec['nbp'] - 1 - spec['revive_after'] < spec['nbp']
    assert run['weights'][spec['nbp'] - 1][hc.DEAD] > 1e-8                 # (and it counts)
    assert numpy.count_nonzero(first == 0) >= 1 and numpy.max(second) == spec['nbp2'] < spec['nbp']
    assert spec['nbp'] > spec['nstblz'] or name != '3x3-spin'               # the re-orthogonalisation inside the window
    for est in run['est']:
        assert numpy.all(numpy.isfinite(est.view(float))) and est[3].real > 0
