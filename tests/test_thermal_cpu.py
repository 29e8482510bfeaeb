"""The finite-temperature path without a GPU: the fp64 restatement (tests/thermal_ref.py) against the fixture recorded
from the genuine reference (tests/golden/thermal_hubbard.npz), the extended-precision restatement against the fp64
one, the trial density matrix and the refusals that need no device."""
import os
import re
import subprocess
import sys

import numpy
import pytest

from tests import thermal_ref as tr
from tests import thermal_ref_ext as te

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERATOR = os.path.join(ROOT, "tests", "golden", "make_golden.py")
ROW_TOL = 1e-9          # golden estimator rows, relative to max(1, max |row|): tests/test_oracle_golden.py


@pytest.fixture(scope="module")
def d(golden):
    return golden("thermal_hubbard.npz")


@pytest.fixture(scope="module")
def paths_a(d):
    """Case (a) once per stack size, in fp64 and in extended precision, on the recorded uniforms: per slice
    (G64, Gx, w64, wx, fields) with the weights scaled as the record is."""
    out = {}
    for k, ss in enumerate(d['a_stack_sizes']):
        L = int(d['a_num_slices'])
        args = (d['a_dmat'], d['a_BH1'], d['a_auxf'], L, int(ss), int(d['a_nstblz']), 1)
        p64 = tr.Path(*args, BT_inv=d['a_dmat_inv'])
        px = te.path(*args, BT_inv=d['a_dmat_inv'])
        rec = [(p64.G.copy(), px.G.copy(), None, None, None)]
        for ts in range(L):
            u = d['a%d_u' % k][ts][None, :]
            f64, fx = p64.step(u), px.step(u)
            p64.weight = p64.weight / d['a_weight_scale']
            px.weight = px.weight / te.LD(d['a_weight_scale'])
            numpy.testing.assert_array_equal(f64, fx)
            rec.append((p64.G.copy(), px.G.copy(), p64.weight.copy(), px.weight.copy(), f64[0]))
        out[k] = (rec, p64, px)
    return out


def test_fixture_margin(d):
    assert float(d['min_margin']) > 1e-6


@pytest.mark.parametrize("k", [0, 1])
def test_restatement_follows_the_reference_walker(d, paths_a, k):
    """Fields exactly; G under the project's rule with the reference in the device's place (both are fp64 evaluations
    of the same unique G): within 100 max(err_ref, 1e-15) of the extended restatement; weights within M x slices x
    that, relative."""
    rec, p64, px = paths_a[k]
    M = d['a_dmat'].shape[-1]
    worst = 0.0
    assert te.gerr(d['a%d_G0' % k], rec[0][1][0]) <= te.bound(te.gerr(rec[0][0], rec[0][1]))
    for ts in range(1, len(rec)):
        G64, Gx, w64, wx, f = rec[ts]
        numpy.testing.assert_array_equal(f, d['a%d_fields' % k][ts - 1])
        err_ref = te.gerr(G64, Gx)
        err_gold = te.gerr(d['a%d_G' % k][ts - 1], Gx[0])
        worst = max(worst, err_gold / te.bound(err_ref))
        assert err_gold <= te.bound(err_ref), (ts, err_ref, err_gold)
        wg = te.ext(d['a%d_weight' % k][ts - 1])
        assert abs(wg / wx[0] - 1) <= M * ts * te.bound(err_ref), (ts, float(abs(wg / wx[0] - 1)))
        assert abs(te.ext(w64[0]) / wx[0] - 1) <= M * ts * te.bound(err_ref)
    print("stack_size %d: largest |reference - extended| / bound = %.3f" % (d['a_stack_sizes'][k], worst))
    H1 = d['a_T']
    E64, nav64 = p64.energy(H1, float(d['a_U']))
    Ex, navx = px.energy(H1, float(d['a_U']))
    scale = float(numpy.max(numpy.sum(numpy.abs(H1[0]), axis=0))) + float(d['a_U']) * M
    bnd = scale * te.bound(te.gerr(p64.G, px.G))
    assert te.gerr(d['a%d_energy' % k], Ex[0]) <= bnd
    assert te.gerr(d['a%d_nav' % k], navx[0]) <= bnd


def test_extended_against_fp64_restatement(paths_a):
    """The two restatements agree to what fp64 loses on this well-conditioned case (4 x 4, U = 4, beta = 2: 1e-15 to
    1e-14 measured against a long-double stratification): 1e-12 leaves the rule's own factor of 100."""
    for k in paths_a:
        rec = paths_a[k][0]
        errs = [te.gerr(r[0], r[1]) for r in rec]
        print("case a%d: err_ref max %.3e" % (k, max(errs)))
        assert max(errs) < 1e-12


def test_restatement_follows_the_reference_driver(d):
    """Case (b): two paths of ThermalAFQMC, 6 walkers, comb every 5 slices, weight cap, reset: the estimator rows."""
    L = int(d['b_ntime_slices'])
    nw = int(d['b_nwalkers'])
    H1 = d['a_T']
    dmat_inv = numpy.array([numpy.linalg.inv(d['b_dmat'][0]), numpy.linalg.inv(d['b_dmat'][1])])
    p = tr.Path(d['b_dmat'], d['b_BH1'], d['b_auxf'], L, int(d['b_stack_size']), int(d['b_nstblz']), nw, BT_inv=dmat_inv)
    rows, used = p.run(d['b_draws'], int(d['b_paths']), int(d['b_npop_control']), H1, float(d['a_U']))
    assert used == len(d['b_draws'])
    assert p.min_margin > 1e-6
    gold = d['blocks'].real
    assert list(d['b_header'][1:11]) == ['WeightFactor', 'Weight', 'ENumer', 'EDenom', 'ETotal', 'E1Body', 'E2Body',
                                          'EHybrid', 'Overlap', 'Nav']
    scale = max(1.0, float(numpy.max(numpy.abs(gold[:, 1:11]))))
    err = float(numpy.max(numpy.abs(rows - gold[:, 1:11]))) / scale
    print("rows: %.3e (tolerance %.1e)" % (err, ROW_TOL))
    assert err <= ROW_TOL


def test_one_body_trial_against_the_reference(d):
    from pauxy_amd.systems import Hubbard
    from pauxy_amd.trial_density import OneBody
    from pauxy_amd.propagation.thermal_hubbard import ThermalDiscrete
    na, nb = [int(x) for x in d['a_nelec']]
    system = Hubbard(4, 4, na, nb, float(d['a_U']), mu=float(d['a_mu_system']))
    assert system.symmetric is False and system._alt_convention is False
    trial = OneBody(system, float(d['a_beta']), float(d['a_dt']))
    assert trial.name == 'thermal'
    assert abs(trial.mu - float(d['a_mu'])) < 1e-12
    assert trial.stack_size == int(d['a_trial_stack_size']) and trial.num_slices == int(d['a_num_slices'])
    assert abs(trial.nav - float(d['a_trial_nav'])) < 1e-10
    numpy.testing.assert_allclose(trial.dmat, d['a_dmat'], rtol=0, atol=1e-14)
    numpy.testing.assert_allclose(trial.dmat_inv, d['a_dmat_inv'], rtol=0, atol=1e-13)

    class Q(object):
        dt, nstblz = float(d['a_dt']), 10
    prop = ThermalDiscrete(system, trial, Q())
    numpy.testing.assert_allclose(prop.auxf, d['a_auxf'], rtol=1e-14)
    numpy.testing.assert_allclose(prop.BH1, d['a_BH1'], rtol=0, atol=1e-14)
    numpy.testing.assert_allclose(tr.hubbard_auxf(float(d['a_U']), Q.dt, system.mu, trial.mu), d['a_auxf'], rtol=1e-14)
    # a fixed chemical potential skips the bisection
    assert OneBody(system, 1.0, 0.05, options={'mu': 0.25}).mu == 0.25


def test_stack_size_estimate_and_update_stack():
    from pauxy_amd.trial_density import update_stack
    assert update_stack(7, 40) == 8 and update_stack(6, 40) == 5 and update_stack(50, 40) == 40 and update_stack(10, 5) == 5


def test_make_golden_thermal_check_reproduces_the_fixture():
    ref = re.search(r'^REF = "(.*)"', open(GENERATOR).read(), re.M).group(1)      # where the generators look for it
    if not (os.path.isdir(ref) and os.access(ref, os.R_OK | os.X_OK)):
        pytest.skip("the reference is not on this machine")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_thermal.py"), "--check"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "all 1 fixtures reproduce" in out.stdout


# ---- refusals that need no device
class _Q(object):
    dt, nstblz, nwalkers, ntot_walkers, beta, nsteps = 0.05, 5, 2, 2, 1.0, 1


def _hubbard_and_trial():
    from pauxy_amd.systems import Hubbard
    from pauxy_amd.trial_density import OneBody
    system = Hubbard(2, 2, 2, 2, 4.0, mu=1.0)
    return system, OneBody(system, 1.0, 0.05, options={'mu': 0.5})


@pytest.mark.parametrize("opts,word", [({'charge_decomposition': True}, 'charge_decomposition'),
                                       ({'free_projection': True}, 'free_projection')])
def test_propagator_options_are_refused(opts, word):
    from pauxy_amd.propagation.thermal_hubbard import ThermalDiscrete
    system, trial = _hubbard_and_trial()
    with pytest.raises(NotImplementedError, match=word):
        ThermalDiscrete(system, trial, _Q(), options=opts)


def test_low_rank_propagator_is_refused():
    from pauxy_amd.propagation.thermal_hubbard import ThermalDiscrete
    system, trial = _hubbard_and_trial()
    with pytest.raises(NotImplementedError, match='low_rank'):
        ThermalDiscrete(system, trial, _Q(), lowrank=True)


@pytest.mark.parametrize("opts,word", [({'low_rank': True}, 'low_rank'), ({'population_control': 'pair_branch'}, 'pair_branch')])
def test_walker_options_are_refused(opts, word):
    from pauxy_amd.walkers.handler import Walkers
    system, trial = _hubbard_and_trial()
    with pytest.raises(NotImplementedError, match=word):
        Walkers(system, trial, _Q(), walker_opts=opts)


def test_more_than_one_rank_is_refused():
    from pauxy_amd.walkers.handler import Walkers
    system, trial = _hubbard_and_trial()

    class TwoRanks(object):
        rank, size = 0, 2
    with pytest.raises(NotImplementedError, match='one rank'):
        Walkers(system, trial, _Q(), comm=TwoRanks())


def test_back_propagation_and_itcf_windows_are_refused():
    from pauxy_amd.walkers.handler import Walkers
    system, trial = _hubbard_and_trial()
    with pytest.raises(NotImplementedError, match='back-propagation or ITCF'):
        Walkers(system, trial, _Q(), nbp=4)
    with pytest.raises(NotImplementedError, match='back-propagation or ITCF'):
        Walkers(system, trial, _Q(), nprop_tot=4)


@pytest.mark.parametrize("opts,word", [({'average_gf': True}, 'average_gf'), ({'one_rdm': True}, 'one_rdm'),
                                       ({'two_rdm': 'structure_factor'}, 'two_rdm')])
def test_mixed_options_are_refused(opts, word):
    from pauxy_amd.estimators.mixed import Mixed
    system, trial = _hubbard_and_trial()
    with pytest.raises(NotImplementedError, match=word):
        Mixed(opts, system, True, None, _Q(), trial)


def test_mixed_has_the_nav_column_before_time():
    from pauxy_amd.estimators.mixed import Mixed
    system, trial = _hubbard_and_trial()
    m = Mixed({}, system, True, None, _Q(), trial)
    assert m.header[-2:] == ['Nav', 'Time'] and m.names.nav == 9 and m.names.time == 10 and m.nreg == 11


def test_generic_ueg_and_mean_field_are_refused():
    from pauxy_amd.propagation.thermal_hubbard import ThermalDiscrete
    from pauxy_amd.qmc.thermal_afqmc import get_trial_density_matrix
    from pauxy_amd.systems import synthetic_generic
    from pauxy_amd.walkers.handler import Walkers
    system, trial = _hubbard_and_trial()
    with pytest.raises(NotImplementedError, match='MeanField'):
        get_trial_density_matrix(system, 1.0, 0.05, options={'name': 'mean_field'})
    generic = synthetic_generic(6, 8, (2, 2), seed=3)
    with pytest.raises(NotImplementedError, match='Generic / UEG'):
        ThermalDiscrete(generic, trial, _Q())
    with pytest.raises(NotImplementedError, match='Generic / UEG'):
        Walkers(generic, trial, _Q())


def test_more_than_64_sites_are_refused_before_the_device():
    from pauxy_amd.systems import Hubbard
    from pauxy_amd.trial_density import OneBody
    from pauxy_amd.walkers.handler import Walkers
    system = Hubbard(9, 8, 30, 30, 4.0, mu=1.0)
    trial = OneBody(system, 1.0, 0.05, options={'mu': 0.5})
    with pytest.raises(NotImplementedError, match='72'):
        Walkers(system, trial, _Q())
