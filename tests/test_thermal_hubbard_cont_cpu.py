"""The finite-temperature Hubbard path with continuous fields, without a GPU: the restatement
(tests/thermal_hubbard_cont_ref.py, fp64 and numpy.clongdouble) against the cases recorded from the genuine reference
(tests/golden/thermal_hubbard_cont.npz), the fixture's generator where the reference is present, the facade's
constants, its refusals, the driver's dispatch, and the host-built table of left_k.

The rule for the restatement is the project's rule for thermal walkers (tests/thermal_ueg_ref_ext.py): with err_ref the
reference's own distance from the extended-precision restatement, the fp64 restatement lies within
100 max(err_ref, 1e-15) of it.  That is what "to the reference's own rounding" means here."""
import os
import re
import subprocess
import sys

import numpy
import pytest

from tests import thermal_hubbard_cont_cases as C
from tests.thermal_ueg_ref_ext import bound, gerr, rerr

HERE = os.path.dirname(os.path.abspath(__file__))


def held(got, ref, want, err=gerr):
    """got (fp64 restatement) against want (extended), the reference's value ref setting the bound."""
    e_ref, e = err(ref, want), err(got, want)
    assert e <= bound(e_ref), (e, e_ref)


def test_fixture_reproduces_from_the_reference():
    """make_golden_thermal_hubbard_cont.py --check: the committed fixture is what the reference gives, margins
    included."""
    gen = os.path.join(HERE, 'golden', 'make_golden_thermal_hubbard_cont.py')
    ref = re.search(r'^REF = "(.*)"', open(os.path.join(HERE, 'golden', 'make_golden.py')).read(), re.M).group(1)
    if not (os.path.isdir(ref) and os.access(ref, os.R_OK | os.X_OK)):
        pytest.skip("the reference is not on this machine")
    run = subprocess.run([sys.executable, gen, '--check'], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and 'identical to the committed fixture' in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]


def test_fixture_covers_what_it_must():
    d = C.golden()
    Ms = sorted(set(int(d['a%d_nx' % k]) * int(d['a%d_ny' % k]) for k in range(C.NA)))
    assert Ms[:3] == [4, 9, 16] and Ms[-1] >= 33
    kinds = set()
    for k in range(C.NA):
        ss = int(d['a%d_stack_size' % k])
        kinds.add('one' if ss == 1 else 'whole' if ss == 10 else 'inner')
    assert kinds == {'one', 'whole', 'inner'}
    assert int(d['a7_nclip']) > 0 and int(d['a7_kills']) > 0
    assert all(int(d['a%d_nclip' % k]) == 0 and int(d['a%d_kills' % k]) == 0 for k in range(7))
    for k in range(C.NB):
        assert int(d['b%d_nclip' % k]) > 0 and int(d['b%d_kills' % k]) > 0 and len(d['b%d_comb_r' % k]) >= 2
        assert numpy.all(numpy.isfinite(d['b%d_blocks' % k]))
    assert float(d['xbar_margin']) > 1e-6


@pytest.mark.parametrize('k', range(C.NA))
def test_restatement_slice_by_slice(k):
    """Case a<k>: the fp64 restatement on the reference's fields, held to the reference's own distance from the
    extended-precision restatement; the clip count and the kills exactly."""
    d = C.golden()
    pre = 'a%d_' % k
    r64, rx = C.ref_run(k, False), C.ref_run(k, True)
    for n in ('xbar', 'cmf', 'cfb'):
        held(r64[n], d[pre + n], rx[n])
    held(r64['G0'], d[pre + 'G0'], rx['G0'])
    held(r64['M00'], d[pre + 'M00'], rx['M00'], rerr)
    if k in C.STORED_G:
        held(r64['G'], d[pre + 'G'], rx['G'])
    held(r64['G'][-1], d[pre + 'G_last'], rx['G'][-1])
    held(r64['M0'], d[pre + 'M0'], rx['M0'], rerr)
    w = d[pre + 'weight']
    alive = w > 0
    held(r64['weight'][alive], w[alive], rx['weight'][alive], rerr)
    assert numpy.all(r64['weight'][~alive] == 0) and numpy.all(rx['weight'][~alive] == 0)
    held(r64['energy'], d[pre + 'energy'], rx['energy'])
    held(r64['nav'], d[pre + 'nav'], rx['nav'])
    for r in (r64, rx):
        assert r['nclip'] == int(d[pre + 'nclip']) and r['nkill'] == int(d[pre + 'kills'])
        assert r['min_cos_margin'] > 1e-6


@pytest.mark.parametrize('k', range(C.NB))
def test_restatement_of_the_driver(k):
    """Driver run b<k>: the comb's parents, the clip count and the kills exactly; rows and per-call weights held to the
    reference's distance from the extended restatement."""
    d = C.golden()
    pre = 'b%d_' % k
    rows64, w64, par64, p64 = C.ref_driver(k, False)
    rowsx, wx, parx, px = C.ref_driver(k, True)
    want = d[pre + 'parent_ix']
    for par in (par64, parx):
        assert len(par) == len(want) and all(numpy.array_equal(a, b) for a, b in zip(par, want))
    for p in (p64, px):
        assert p.nclip == int(d[pre + 'nclip']) and p.nkill == int(d[pre + 'kills'])
    ref_rows = d[pre + 'blocks'][:, 1:11].real
    cols = [0, 1, 2, 3, 4, 5, 6, 9]                # (EHybrid is 0 and Overlap 1 in every row)
    held(rows64[:, cols], ref_rows[:, cols], rowsx[:, cols], rerr)
    assert numpy.all(rows64[:, 7] == 0) and numpy.all(rows64[:, 8] == 1)
    ref_w = d[pre + 'weights']
    alive = ref_w > 0
    held(w64[alive], ref_w[alive], wx[alive], rerr)
    assert numpy.all(w64[~alive] == 0) and numpy.all(wx[~alive] == 0)


@pytest.mark.parametrize('k', [0, 2, 4, 6, 7])
def test_facade_constants_against_the_fixture(k):
    """Continuous(options, qmc, system, trial): the reference's argument order and attributes.  The constants come from
    scipy's expm and inv on both sides: 1e-13 on the scale of the quantity leaves room for a different LAPACK only."""
    from pauxy_amd.propagation.thermal_continuous import Continuous
    d = C.golden()
    pre = 'a%d_' % k
    system, trial = C.system_and_trial(pre)
    dt = float(d[pre + 'dt'])
    prop = Continuous({}, C.Qmc(dt), system, trial, verbose=False, lowrank=False)
    assert abs(trial.mu - float(d[pre + 'mu'])) < 1e-12
    assert gerr(trial.dmat, d[pre + 'dmat']) < 1e-13 and gerr(trial.dmat_inv, d[pre + 'dmat_inv']) < 1e-13
    assert prop.BH1.dtype == numpy.float64 and prop.BH1.shape == (2, system.nbasis, system.nbasis)
    assert gerr(prop.BH1, d[pre + 'BH1']) < 1e-13
    assert gerr(prop.propagator.mf_shift, d[pre + 'mf_shift']) < 1e-13
    assert abs(prop.propagator.mf_core / complex(d[pre + 'mf_core']) - 1) < 1e-13
    assert abs(prop.mf_const_fac / complex(d[pre + 'mf_const_fac']) - 1) < 1e-12
    assert prop.hs_type == 'continuous' and prop.exp_nmax == 6 and prop.dt == dt
    assert prop.sqrt_dt == dt ** 0.5 and prop.isqrt_dt == 1j * dt ** 0.5
    assert prop.nfb_trig == 0 and isinstance(prop.nfb_trig, int)
    assert prop.lowrank is False and prop.free_projection is False and prop.force_bias is True
    assert prop.propagator.iu_fac == 1j * float(d[pre + 'U']) ** 0.5
    assert prop.propagator.BH1 is prop.BH1 and prop.BT is trial.dmat and prop.BTinv is trial.dmat_inv
    assert prop.BT_BP is None and prop.mu == system.mu and prop.nstblz == 10
    assert prop.ebound == (2.0 / dt) ** 0.5
    # the restatement's own constants agree with both
    BH1, mf_shift, mf_core, mfc = C.R.constants(system.T[0], system.U, system.mu, dt, numpy.asarray(trial.dmat.real))
    assert gerr(BH1, d[pre + 'BH1']) < 1e-13 and gerr(mf_shift, d[pre + 'mf_shift']) < 1e-13
    assert abs(mfc / complex(d[pre + 'mf_const_fac']) - 1) < 1e-12


def hubbard_and_trial():
    from pauxy_amd.systems import Hubbard
    from pauxy_amd.trial_density import OneBody
    system = Hubbard(2, 2, 2, 2, 4.0, mu=1.0)
    return system, OneBody(system, 0.5, 0.05)


@pytest.mark.parametrize('options, lowrank, word', [
    ({'free_projection': True}, False, 'free_projection'),
    ({'force_bias': False}, False, 'force_bias'),
    ({}, True, 'low_rank'),
    ({'low_rank': True}, False, 'low_rank'),
    ({'expansion_order': 4}, False, 'expansion_order'),
])
def test_refusals_by_word(options, lowrank, word):
    from pauxy_amd.propagation.thermal_continuous import Continuous
    system, trial = hubbard_and_trial()
    with pytest.raises(NotImplementedError, match=word):
        Continuous(options, C.Qmc(0.05), system, trial, lowrank=lowrank)


def test_refuses_other_systems_trials_and_conventions():
    from pauxy_amd.propagation.thermal_continuous import Continuous
    from pauxy_amd.systems import UEG
    system, trial = hubbard_and_trial()
    ueg = UEG(1.0, 1, 1, 0.5, full_lists=True)
    ueg.mu = 0.245
    with pytest.raises(NotImplementedError, match='Hubbard systems only'):
        Continuous({}, C.Qmc(0.05), ueg, trial)

    class Generic(object):
        name = "Generic"
    with pytest.raises(NotImplementedError, match='Generic'):
        Continuous({}, C.Qmc(0.05), Generic(), trial)

    class MeanField(object):
        name = 'thermal'
    with pytest.raises(NotImplementedError, match='OneBody'):
        Continuous({}, C.Qmc(0.05), system, MeanField())
    system.symmetric = True
    with pytest.raises(NotImplementedError, match='symmetric'):
        Continuous({}, C.Qmc(0.05), system, trial)
    system.symmetric = False
    system._alt_convention = True
    with pytest.raises(NotImplementedError, match='convention'):
        Continuous({}, C.Qmc(0.05), system, trial)


def test_a_bh1_with_an_imaginary_part_is_refused_by_name():
    """A complex hopping matrix makes expm complex: the facade refuses it instead of dropping the imaginary part."""
    from pauxy_amd.propagation.thermal_continuous import Continuous
    system, trial = hubbard_and_trial()
    T = numpy.array(system.h1e_mod, dtype=numpy.complex128)
    T[:, 0, 1] += 0.3j
    T[:, 1, 0] -= 0.3j
    system.h1e_mod = T
    with pytest.raises(NotImplementedError, match='imaginary'):
        Continuous({}, C.Qmc(0.05), system, trial)


def test_get_propagator_dispatch():
    """Hubbard: 'discrete' and no key give ThermalDiscrete (the default does not move); anything else Continuous."""
    from pauxy_amd.propagation.thermal_continuous import Continuous
    from pauxy_amd.propagation.thermal_hubbard import ThermalDiscrete
    from pauxy_amd.qmc.thermal_afqmc import get_propagator
    system, trial = hubbard_and_trial()
    q = C.Qmc(0.05)
    assert type(get_propagator(system, trial, q, {})) is ThermalDiscrete
    assert type(get_propagator(system, trial, q, {'hubbard_stratonovich': 'discrete'})) is ThermalDiscrete
    for name in ('continuous', 'generic'):
        prop = get_propagator(system, trial, q, {'hubbard_stratonovich': name})
        assert type(prop) is Continuous and prop.hs_type == 'continuous'
    with pytest.raises(NotImplementedError, match='free_projection'):
        get_propagator(system, trial, q, {'hubbard_stratonovich': 'continuous', 'free_projection': True})


@pytest.mark.parametrize('k', C.STORED_G)
def test_host_built_left_table_is_the_references_bit_for_bit(k):
    """left_k of the library's host code (afq_thermal_left_table, what the configuration uploads) against the
    reference's stack.left after every slice of case a<k>: the same bits."""
    from pauxy_amd import _lib
    from pauxy_amd.propagation.thermal_continuous import left_table
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    d = C.golden()
    pre = 'a%d_' % k
    ss = int(d[pre + 'stack_size'])
    pw, left = left_table(d[pre + 'dmat'], d[pre + 'dmat_inv'], ss)
    ref = d[pre + 'left']
    assert ref.shape == (10,) + left.shape[1:] and ref.dtype == numpy.float64
    for ts in range(10):
        assert numpy.array_equal(left[ts % ss], ref[ts]), ts
    # the restatement builds the same table in the same order: up to 2 stack_size products of inner dimension M, each
    # rounding M eps at the most on the scale of the result
    p = C.ref_path(pre, C.Kit64)
    tol = 2 * ss * left.shape[-1] * numpy.finfo(float).eps
    assert gerr(numpy.array(p.left_table), left) < tol and gerr(p.BTpow, pw) < tol
