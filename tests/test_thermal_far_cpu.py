"""The far route of the complex thermal walkers (AFQ_THERMAL_FAR, walkers: {far_basis: True}) without a GPU: the fp64
restatement replays the two fixtures recorded from the reference where only that route runs (thermal_ueg123.npz,
thermal_hubbard_cont_far.npz) under the thermal tests' rule, at the tolerance tests/test_thermal_wide_cpu.py uses at
M = 93 -- the fp64 restatement lies within 100 max(err_ref, 1e-15) of the extended one, err_ref the reference's own
distance from it -- with the extended results read from the stored files and their first slice recomputed here; the
walkers' bounds and refusals around the option before any device is touched; the header's bit and the library's bound."""
import os
import re
import types

import numpy
import pytest

from pauxy_amd import _lib as L
from tests import thermal_far_cases as F
from tests import thermal_ueg_ref_ext as ue
from tests import thermal_wide_cases as W
from tests.test_thermal_wide_cpu import first_slice_is_what_is_stored, held, replay

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("gen", ["make_golden_thermal_ueg_far.py", "make_golden_thermal_hubbard_cont_far.py"])
def test_fixture_reproduces_from_the_reference(gen):
    """--check of the generator: the committed fixture is what the reference gives, margins and the seed search
    included (one BLAS thread: at these sizes a threaded one is the slower)."""
    import subprocess
    import sys
    ref = re.search(r'^REF = "(.*)"', open(os.path.join(HERE, 'golden', 'make_golden.py')).read(), re.M).group(1)
    if not (os.path.isdir(ref) and os.access(ref, os.R_OK | os.X_OK)):
        pytest.skip("the reference is not on this machine")
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    run = subprocess.run([sys.executable, os.path.join(HERE, 'golden', gen), '--check'], capture_output=True, text=True,
                         timeout=600, env=env)
    assert run.returncode == 0 and 'identical to the committed fixture' in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]


def test_extended_restatements_reproduce():
    """make_thermal_far_ext.py is checked by parts here (first slices below); its files are within the size of a
    committed file and hold every key the GPU tests read."""
    x = F.stored_ext()
    for name in list(F.EXT_OF) + list(F.EXT_OF.values()) + [F.BINS_EXT]:
        assert os.path.getsize(os.path.join(HERE, 'golden', name)) <= 1024 * 1024, name
    for key in ('a8_G', 'a8_M00', 'a8_energy', 'b6_wx', 'b6_rx', 'h10_G_last', 'h10_M00', 'hb3_wx', 'hb3_rx'):
        assert key + '_hi' in x and key + '_lo' in x, key
    for key in ('a8_right', 'a8_bin', 'h10_right', 'h10_bin'):
        assert key + '_hi' in x and key + '_lo' in x, key
    assert 'b6_parents' in x and 'hb3_parents' in x


def test_ueg_123_through_both_restatements():
    d, x = F.golden(F.UEG), F.stored_ext()
    pre = F.UEG_A
    c = W.case_of_fixture(d, pre)
    assert c.M == 123 and c.L == 10 and int(d[pre + 'stack_size']) == 5 and list(d[pre + 'G_slices']) == [10]
    assert d[pre + 'G'].shape == (1, 2, 123, 123) and d[pre + 'xi'].shape == (10, c.K)
    replay(pre, d, pre, W.ueg_run(F.UEG, pre, False), x, pre, 'G')
    first_slice_is_what_is_stored(pre, W.ueg_run(F.UEG, pre, True, nslice=1), x, pre)


def test_hubbard_8x16_through_both_restatements():
    d, x = F.golden(F.HUBBARD), F.stored_ext()
    pre, xpre = 'a%d_' % F.HUBBARD_A, 'h%d_' % F.HUBBARD_A
    assert (int(d[pre + 'nx']), int(d[pre + 'ny'])) == (8, 16) and int(d[pre + 'stack_size']) == 5
    assert pre + 'G' not in d and d[pre + 'G_last'].shape == (2, 128, 128) and d[pre + 'dmat'].shape == (1, 128, 128)
    replay(pre, d, pre, F.hubbard_run(False), x, xpre, 'G_last')
    first_slice_is_what_is_stored(pre, F.hubbard_run(True, nslice=1), x, xpre)


def test_ueg_driver_at_123_against_the_stored_extended_run():
    """Case b6: the comb's parents of the reference and of the stored extended run are the same, a walker is cloned, and
    the reference's rows and weights lie within 1e-10 of the extended run's (the single-walker case above replays this
    basis slice by slice in fp64)."""
    d, x = F.golden(F.UEG), F.stored_ext()
    pre = 'b%d_' % F.UEG_B
    assert int(d[pre + 'seed']) >= 8 and int(d[pre + 'nwalkers']) == 4 and numpy.any(d[pre + 'parent_ix'] > 1)
    numpy.testing.assert_array_equal(d[pre + 'parent_ix'], x[pre + 'parents'])
    wx, rx = F.joined(x, pre + 'wx'), F.joined(x, pre + 'rx')
    assert wx.shape == d[pre + 'weights'].shape == (20, 4) and rx.shape == (3, 10)
    assert ue.rerr(d[pre + 'weights'], wx) <= 1e-10
    assert ue.gerr(d[pre + 'blocks'].real[:, 1:11], rx, max(1.0, float(numpy.max(numpy.abs(rx))))) <= 1e-10


@pytest.mark.parametrize("which,xpre,M", [('ueg', F.UEG_A, 123), ('hubbard', 'h%d_' % F.HUBBARD_A, 128)])
def test_stored_bins_and_right(which, xpre, M):
    """What the slice kernels write, as stored for the GPU tests: the fp64 restatement within 1e-12 of the stored
    extended rows at every stored slice (products of order 128 over at most five slices of a bin: some M eps each, on
    the scale of the largest element), and the first stored slice of the extended restatement recomputed bit for bit."""
    x = F.stored_ext()
    rows = F.bin_rows(M)
    assert rows[0] == 0 and rows[-1] == M - 1 and F.BIN_SLICES == (2, 6, 10)
    r64 = F.bins_run(which, False)
    for q in ('right', 'bin'):
        want = F.joined(x, xpre + q)
        assert want.shape == (3, 2, len(rows), M) == r64[q].shape
        for i, ts in enumerate(F.BIN_SLICES):
            scale = max(1.0, float(numpy.max(numpy.abs(ue.ext(want[i])))))
            err = ue.gerr(r64[q][i], want[i], scale)
            print("%s slice %d %s: fp64 restatement %.3e" % (which, ts, q, err))
            assert err <= 1e-12, (which, ts, q, err)
    rx = F.bins_run(which, True, upto=F.BIN_SLICES[0])
    for q in ('right', 'bin'):
        hi, lo = F.split(rx[q], small=True)
        numpy.testing.assert_array_equal(hi[0], x[xpre + q + '_hi'][0])
        numpy.testing.assert_array_equal(lo[0], x[xpre + q + '_lo'][0])


def test_ueg_driver_at_123_through_the_fp64_restatement():
    """Case b6 replayed: fields and comb uniforms from the seed through the fp64 restatement: the reference's parents,
    and its rows and per-slice weights under the rule against the stored extended run."""
    from tests.golden.make_thermal_ueg_paths_ext import run_case
    d, x = F.golden(F.UEG), F.stored_ext()
    pre = 'b%d_' % F.UEG_B
    b = run_case(d, F.UEG_B, kits=('fp64',))
    held("b6 weights", b[pre + 'w64'], d[pre + 'weights'], F.joined(x, pre + 'wx'), relative=True)
    held("b6 rows", b[pre + 'r64'], d[pre + 'blocks'].real[:, 1:11], F.joined(x, pre + 'rx'))


def test_hubbard_driver_on_10x10_through_the_fp64_restatement():
    d, x = F.golden(F.HUBBARD), F.stored_ext()
    pre, xp = 'b%d_' % F.HUBBARD_B, 'hb%d_' % F.HUBBARD_B
    assert int(d[pre + 'nx']) == int(d[pre + 'ny']) == 10 and int(d[pre + 'nwalkers']) == 4
    rows, wts, parents, p = F.hubbard_driver(False)
    numpy.testing.assert_array_equal(numpy.array(parents), d[pre + 'parent_ix'])
    numpy.testing.assert_array_equal(numpy.array(parents), x[xp + 'parents'])
    assert p.nclip == int(d[pre + 'nclip'])
    ref_w, wx = d[pre + 'weights'], F.joined(x, xp + 'wx')
    alive = ref_w > 0
    assert numpy.all(numpy.asarray(wts)[~alive] == 0) and numpy.all(wx[~alive] == 0)
    held("b3 weights", numpy.asarray(wts)[alive], ref_w[alive], wx[alive], relative=True)
    cols = [0, 1, 2, 3, 4, 5, 6, 9]                    # (EHybrid is 0 and Overlap 1 in every row)
    held("b3 rows", numpy.asarray(rows)[:, cols], d[pre + 'blocks'].real[:, 1:11][:, cols], F.joined(x, xp + 'rx')[:, cols],
         relative=True)


def test_the_observables_fixture_has_the_averaged_runs_the_sweep_tests_repeat():
    """tests/test_gpu_thermal_sweep_routes.py repeats the `average_gf` runs of thermal_obs.npz on complex walkers: the
    UEG at M = 19 and 7 and the 3 x 3 lattice with continuous fields are among them."""
    from tests import thermal_obs_ref as R
    tags = [tag for tag in R.MODELS if R.MODELS[tag][0] != 'hubbard' and R.numbers(tag)['average_gf']]
    assert sorted(tags) == ['hc', 'ub', 'uc', 'ud'] and R.MODELS['hc'][0] == 'hubbard_continuous'
    assert {R.MODELS[t][1].get('ecut') for t in tags if R.MODELS[t][0] == 'ueg'} == {1.0, 0.5}


# ---- the header, the library, the walkers
def test_header_defines_the_bit_and_the_library_exports_the_bound():
    text = open(os.path.join(os.path.dirname(HERE), 'include', 'afqmc_hip.h')).read()
    assert re.search(r'^#define AFQ_THERMAL_FAR\s+256\b', text, re.M)
    assert re.search(r'^int afq_thermal_far_max_basis\(void\);', text, re.M)
    others = L.THERMAL_WIDE | L.THERMAL_STREAMED_GREENS | L.THERMAL_DELAYED | 15 | 64       # (64 stays the unknown bit)
    assert L.THERMAL_FAR == 256 and L.THERMAL_FAR & others == 0
    assert int(L.load().afq_thermal_far_max_basis()) == 128


def test_max_basis_has_a_far_column_read_from_the_library():
    from pauxy_amd.walkers.thermal import MAX_BASIS
    M = int(L.load().afq_thermal_far_max_basis())
    assert MAX_BASIS['planewave', 'far'] == MAX_BASIS['hubbard_continuous', 'far'] == M == 128
    assert MAX_BASIS['planewave', 'wide'] == MAX_BASIS['hubbard_continuous', 'wide'] == 95


def test_check_bound_words_the_far_bound():
    from pauxy_amd.walkers.thermal import ThermalWalkers
    me = types.SimpleNamespace(wide_basis=False, streamed_greens=False, far_basis=True)
    for kind, unit in (('planewave', 'plane waves'), ('hubbard_continuous', 'sites')):
        for M in (64, 96, 123, 128):
            ThermalWalkers._check_bound(me, kind, M)
        with pytest.raises(NotImplementedError) as e:
            ThermalWalkers._check_bound(me, kind, 129)
        text = str(e.value)
        assert "M = 129 > 128 %s" % unit in text and "far_basis" in text and "two columns" in text


class Q(object):
    dt, nstblz, nwalkers, ntot_walkers = 0.05, 5, 2, 2


def test_walkers_refuse_far_basis_before_the_device():
    """On discrete fields by name; together with wide_basis and with streamed_greens; at M = 129 with the numbers."""
    from pauxy_amd.systems import UEG, Hubbard
    from pauxy_amd.trial_density import OneBody
    from pauxy_amd.walkers.handler import Walkers
    system = Hubbard(2, 2, 2, 2, 4.0, mu=1.0)
    trial = OneBody(system, 1.0, 0.05, options={'mu': 0.5})
    with pytest.raises(NotImplementedError, match='far_basis belongs to the continuous fields'):
        Walkers(system, trial, Q(), walker_opts={'far_basis': True})
    with pytest.raises(NotImplementedError, match='far_basis and wide_basis are two placements'):
        Walkers(system, trial, Q(), walker_opts={'far_basis': True, 'wide_basis': True, 'continuous_fields': True})
    with pytest.raises(NotImplementedError, match='far_basis and streamed_greens are two placements'):
        Walkers(system, trial, Q(), walker_opts={'far_basis': True, 'streamed_greens': True, 'continuous_fields': True})
    system = Hubbard(129, 1, 56, 56, 4.0, mu=1.0)
    trial = OneBody(system, 0.5, 0.05, options={'mu': 0.5})
    with pytest.raises(NotImplementedError, match='M = 129 > 128 sites'):
        Walkers(system, trial, Q(), walker_opts={'far_basis': True, 'continuous_fields': True})
    system = UEG(1.0, 2, 2, 5.0, full_lists=True)
    system.mu = 0.245
    assert system.nbasis > 128
    with pytest.raises(NotImplementedError, match='M = %d > 128 plane waves' % system.nbasis):
        Walkers(system, OneBody(system, 0.5, 0.05), Q(), walker_opts={'stack_size': 5, 'far_basis': True})
