"""The fixtures of tests/test_gpu_constraint_edges.py, checked on the reference alone: every named case of
tests/constraint_cases.py reaches the branches of the phaseless constraint it is meant to reach (force-bias bound on 10 % to
90 % of the live (walker, field) pairs, at least two walkers above, below and inside the energy bound, at least 20 % of
the live walkers killed by their phase and 20 % surviving), no decision is closer than 1e-6 to its threshold, dead walkers
are present and left alone, the counts the oracle returns are the sums of its masks, and the reference's own result does
not move by more than 1e-11 when a walker is perturbed by one rounding error.  Run with -s for the branch
counts per case."""
import numpy
import pytest

from oracle import afqmc_ref as ref
from tests import constraint_cases as cc


@pytest.mark.parametrize("name", cc.names())
def test_case_reaches_its_branches(name):
    run = cc.run_oracle(name)
    model, phis, weights, xi, eshift, extra = run['case']
    s = cc.check_case(name, run['case'], run['verdicts'])
    print("\n%s: M=%d K=%d %d+%d nw=%d live=%d | clipped %d/%d pairs (%.0f %%), walkers without / with some clipped "
          "fields %d / %d | energy bound above/inside/below %d/%d/%d (nhe %d) | killed %d (%.0f %%) survived %d | "
          "margins fb %.1e e %.1e cos %.1e"
          % (name, model.M, model.nfields, model.na, model.nb, s['nw'], s['live'], s['clipped'], s['pairs'],
             100.0 * s['clipped'] / s['pairs'], s['walkers_unclipped'], s['walkers_mixed'], s['above'], s['inside'],
             s['below'], s['nhe'], s['killed'], 100.0 * s['killed'] / s['live'], s['survived'], s['margin_fb'],
             s['margin_e'], s['margin_cos']))
    first = run['verdicts'][0]
    for vs in run['verdicts']:
        for v in vs:
            if not v['live']:
                continue
            # the oracle's counts are the sums of the masks
            assert v['nfb'] == int(v['mask'].sum())
            assert v['nhe'] == (1 if v['side'] != 0 else 0)
            # clipped fields have modulus 1, the others are the force bias itself
            assert numpy.max(numpy.abs(numpy.abs(v['xbar'][v['mask']]) - 1.0), initial=0.0) < 1e-14
            assert numpy.allclose(v['xbar'][~v['mask']], v['xbar_raw'][~v['mask']], rtol=0, atol=1e-13)
            # a bounded energy sits on the bound with its imaginary part kept, a killed walker has weight exactly 0
            e = v['hybrid_energy'] if extra['hybrid'] else None
            if e is not None and v['side'] != 0:
                assert e.real == eshift + v['side'] * (2.0 / model.dt) ** 0.5 and e.imag == v['e_unbounded'].imag
            if v['cos'] <= 0.0:
                assert v['weight'] == 0.0
    # walkers that start dead come back untouched; the ones a step kills are not propagated by the next
    for i, v in enumerate(first):
        if not v['live']:
            assert numpy.array_equal(v['phi'], phis[i]) and v['weight'] == weights[i]
        if v['weight'] == 0.0:
            assert not run['verdicts'][1][i]['live']
            assert numpy.array_equal(run['verdicts'][1][i]['phi'], v['phi'])
    if abs(eshift) < 1e-10:
        assert all(v['nhe'] == 0 for vs in run['verdicts'] for v in vs if v['live'])
    if extra['cap'] is not None:
        top = extra['cap'][0] * extra['cap'][1]
        assert sum(1 for v in first if v['weight'] == top) >= 2 and all(v['weight'] <= top for v in first)


@pytest.mark.parametrize("name", cc.names())
def test_case_is_well_conditioned(name):
    """One rounding error in a walker moves nothing the device tests compare by more than a hundredth of their
    tolerance, and flips no decision: what those tests see is the code, not the rounding history of an ill-conditioned
    fixture."""
    worst = cc.sensitivity(name)
    print("\n%s: one unit in the last place of a walker moves the reference's step by %.1e" % (name, worst))
    assert worst <= cc.CONDITIONING, (name, worst)


def test_unshifted_twin_has_the_same_population():
    """The same population once more with eshift = 0: the energies the bound would look at are the same numbers, and
    none is bounded."""
    for a, b in (('tiny-open', 'tiny-open-noshift'), ('hubbard-charge', 'hubbard-charge-noshift')):
        va, vb = cc.run_oracle(a)['verdicts'][0], cc.run_oracle(b)['verdicts'][0]
        assert sum(v['nhe'] for v in va if v['live']) > 0
        for x, y in zip(va, vb):
            assert x['live'] == y['live']
            if x['live']:
                assert x['e_unbounded'] == y['e_unbounded'] and y['nhe'] == 0 and y['hybrid_energy'] == y['e_unbounded']


def test_overflow_case_takes_both_ends():
    """e_old = -1e6: infinite importance function, weight 0, nothing recorded for back-propagation (the reference's
    ``if not math.isinf(magn)``); e_old = +1e6: it underflows to 0, weight 0, the recorded factors are (0, 0)."""
    run = cc.run_oracle('overflow')
    model, phis, weights, xi, eshift, extra = run['case']
    first = run['verdicts'][0]
    live = [i for i, v in enumerate(first) if v['live']]
    inf = [i for i in live if extra['ehyb0'][i].real == -1e6]
    zero = [i for i in live if extra['ehyb0'][i].real == 1e6]
    assert all(first[i]['weight'] == 0.0 and numpy.isfinite(first[i]['hybrid_energy']) for i in inf + zero)
    # the window: the walkers of the infinite end recorded no step, the others one (they are dead in the second step)
    assert list(run['bp_steps'][inf]) == [0] * len(inf) and list(run['bp_steps'][zero]) == [1] * len(zero)
    assert numpy.all(numpy.isfinite(run['bp_est']))
    # the oracle's weight update on its own, both ends
    for e_old, wfac in ((-1e6, None), (1e6, (0.0, 0.0))):
        w = dict(weight=1.0, ot=1.0 + 0j, ovlp=1.0 + 0j, hybrid_energy=e_old)
        assert ref.update_weight_hybrid(w, 1.0 + 0j, 0.9 + 0.1j, 0.0, 0.0, 0.0, 0.01) == 0
        assert w['weight'] == 0.0 and w['_wfac'] == wfac and w['ot'] == 0.9 + 0.1j
