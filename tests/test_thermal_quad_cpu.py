"""The quad route of the complex thermal walkers (AFQ_THERMAL_QUAD, walkers: {quad_basis: True}) without a GPU: the
fixtures recorded from the reference where only that route runs (thermal_ueg147.npz, thermal_hubbard_cont_quad.npz) and
their stored extended restatements -- they exist, stay within the size of a committed file, and the fp64 restatement
replays them under the thermal tests' rule (within 100 max(err_ref, 1e-15) of the extended one, err_ref the reference's own
distance from it; the two records of one path within 1e-10) with the first slice of the extended restatement recomputed
bit for bit; the stored Green's functions alone at M = 129, 193, 256, whose fp64 restatement lies within 1e-13 of them
(their bins are rebuilt by fp64 products on every machine: the smallest is recomputed to 1e-14, not to the bit);
the header's bit and the library's bound; the walkers' bounds and refusals around the option before any device is
touched."""
import os
import re
import types

import numpy
import pytest

from pauxy_amd import _lib as L
from tests import thermal_quad_cases as Q
from tests import thermal_wide_cases as W
from tests.test_thermal_wide_cpu import first_slice_is_what_is_stored, held, replay

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_BYTES = 1024 * 1024


@pytest.mark.parametrize("gen", ["make_golden_thermal_ueg_quad.py", "make_golden_thermal_hubbard_cont_quad.py"])
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


def test_fixtures_exist_within_the_size_of_a_committed_file_and_hold_the_keys():
    x = Q.stored_ext()
    for name in list(Q.EXT_OF) + list(Q.EXT_OF.values()) + [Q.GREENS_EXT]:
        assert os.path.getsize(os.path.join(HERE, 'golden', name)) <= MAX_BYTES, name
    for key in ('a9_G', 'a9_M00', 'a9_energy', 'b7_wx', 'b7_rx', 'h11_G_last', 'h11_bins_last', 'h11_right_last', 'h11_M00',
                'hb4_wx', 'hb4_rx'):
        assert key + '_hi' in x and key + '_lo' in x, key
    assert 'b7_parents' in x and 'hb4_parents' in x
    for M, nbins in Q.GREENS_CASES:
        key = Q.greens_key(M, nbins)
        assert x[key + 'G_hi'].shape == (2, len(Q.rows_of(M)), M) and x[key + 'det_hi'].shape == (2,)
        numpy.testing.assert_array_equal(x[key + 'rows'], Q.rows_of(M))
    assert list(Q.rows_of(256)) == [0, 63, 64, 127, 128, 191, 192, 255] and list(Q.rows_of(129)) == [0, 63, 64, 127, 128]
    assert {M for M, _ in Q.GREENS_CASES} == {129, 193, 256} and {n for _, n in Q.GREENS_CASES} == {2, 5}


def test_ueg_147_through_both_restatements():
    d, x = Q.golden(Q.UEG), Q.stored_ext()
    pre = Q.UEG_A
    c = W.case_of_fixture(d, pre)
    assert c.M == 147 and c.L == 10 and int(d[pre + 'stack_size']) == 5 and list(d[pre + 'G_slices']) == [10]
    assert d[pre + 'G'].shape == (1, 2, 147, 147) and d[pre + 'xi'].shape == (10, c.K)
    rows = x[pre + 'G_rows']                            # (the extended file holds these rows of G)
    numpy.testing.assert_array_equal(rows, Q.ueg_g_rows(147))
    assert len(rows) == 76 and set(Q.rows_of(147)) <= set(rows)
    r64 = W.ueg_run(Q.UEG, pre, False)
    r64['G'] = r64['G'][:, :, rows]
    replay(pre, dict(d, **{pre + 'G': d[pre + 'G'][:, :, rows]}), pre, r64, x, pre, 'G')
    first_slice_is_what_is_stored(pre, W.ueg_run(Q.UEG, pre, True, nslice=1), x, pre)


def test_hubbard_16x16_through_the_fp64_restatement():
    """Case a11 on the stored rows: the scalars of every slice, and G, both bins and right behind the last slice, replay
    under the rule (the first slice of the extended restatement at M = 256 is recomputed by
    make_thermal_quad_ext.py --check: it takes a minute)."""
    d, x = Q.golden(Q.HUBBARD), Q.stored_ext()
    pre, xpre = 'a%d_' % Q.HUBBARD_A, 'h%d_' % Q.HUBBARD_A
    assert (int(d[pre + 'nx']), int(d[pre + 'ny'])) == (16, 16) and int(d[pre + 'stack_size']) == 5
    assert list(d[pre + 'rows']) == list(Q.rows_of(256))
    assert d[pre + 'G_last'].shape == (2, 8, 256) and d[pre + 'bins_last'].shape == (2, 2, 8, 256)
    assert d[pre + 'right_last'].shape == (2, 8, 256) and d[pre + 'dmat'].shape == (1, 256, 256)
    r64 = Q.hubbard_run(False)
    replay(pre, d, pre, r64, x, xpre, 'G_last')
    held("a11 bins", r64['bins_last'], d[pre + 'bins_last'], W.joined(x, xpre + 'bins_last'))
    held("a11 right", r64['right_last'], d[pre + 'right_last'], W.joined(x, xpre + 'right_last'))


def test_ueg_driver_at_147_through_the_fp64_restatement():
    """Case b7 replayed: fields and comb uniforms from the seed through the fp64 restatement: the reference's parents (a
    walker is cloned), and its rows and per-slice weights under the rule against the stored extended run."""
    from tests.golden.make_thermal_ueg_paths_ext import run_case
    d, x = Q.golden(Q.UEG), Q.stored_ext()
    pre = 'b%d_' % Q.UEG_B
    assert int(d[pre + 'nwalkers']) == 4 and numpy.any(d[pre + 'parent_ix'] > 1)
    numpy.testing.assert_array_equal(d[pre + 'parent_ix'], x[pre + 'parents'])
    b = run_case(d, Q.UEG_B, kits=('fp64',))
    held("b7 weights", b[pre + 'w64'], d[pre + 'weights'], W.joined(x, pre + 'wx'), relative=True)
    held("b7 rows", b[pre + 'r64'], d[pre + 'blocks'].real[:, 1:11], W.joined(x, pre + 'rx'))


def test_hubbard_driver_on_12x12_through_the_fp64_restatement():
    d, x = Q.golden(Q.HUBBARD), Q.stored_ext()
    pre, xp = 'b%d_' % Q.HUBBARD_B, 'hb%d_' % Q.HUBBARD_B
    assert int(d[pre + 'nx']) == int(d[pre + 'ny']) == 12 and int(d[pre + 'nwalkers']) == 4
    rows, wts, parents, p = Q.hubbard_driver(False)
    numpy.testing.assert_array_equal(numpy.array(parents), d[pre + 'parent_ix'])
    numpy.testing.assert_array_equal(numpy.array(parents), x[xp + 'parents'])
    assert p.nclip == int(d[pre + 'nclip'])
    ref_w, wx = d[pre + 'weights'], W.joined(x, xp + 'wx')
    alive = ref_w > 0
    assert numpy.all(numpy.asarray(wts)[~alive] == 0) and numpy.all(wx[~alive] == 0)
    held("b4 weights", numpy.asarray(wts)[alive], ref_w[alive], wx[alive], relative=True)
    cols = [0, 1, 2, 3, 4, 5, 6, 9]                    # (EHybrid is 0 and Overlap 1 in every row)
    held("b4 rows", numpy.asarray(rows)[:, cols], d[pre + 'blocks'].real[:, 1:11][:, cols], W.joined(x, xp + 'rx')[:, cols],
         relative=True)


@pytest.mark.parametrize("M,nbins", Q.GREENS_CASES)
def test_stored_greens_functions_replay_through_the_fp64_restatement(M, nbins):
    """The fp64 restatement of the Green's function alone lies where the file says it does: its distance from the stored
    extended rows within a factor 2 of the stored err64 (the fp64 path goes through LAPACK) and below 1e-13; the
    determinants' likewise, relative."""
    x = Q.stored_ext()
    key = Q.greens_key(M, nbins)
    G64, det64 = Q.greens_run(M, nbins, False)
    eg, ed = Q.err_of(G64, W.joined(x, key + 'G')), Q.err_of(det64, W.joined(x, key + 'det'), relative=True)
    print("%s fp64 restatement: G %.3e (stored %.3e) det %.3e (stored %.3e)" % (key, eg, float(x[key + 'G_err64']), ed,
                                                                               float(x[key + 'det_err64'])))
    assert eg <= 2 * float(x[key + 'G_err64']) + 1e-15 and eg <= 1e-13
    assert ed <= 2 * float(x[key + 'det_err64']) + 1e-15 and ed <= 1e-13


def test_smallest_stored_greens_function_recomputes():
    """make_thermal_quad_ext.py is checked by parts here: M = 129 with 2 bins through the extended restatement.  The bins
    are rebuilt here by fp64 matrix products, whose last bit depends on the BLAS and its threads, so the recomputed
    result is held to the stored one to 1e-14 (G, on its scale) and 1e-13 (det, relative: 129 pivots), not to the bit:
    an input moved by an ulp moves G by what err64 measures."""
    x = Q.stored_ext()
    key = Q.greens_key(129, 2)
    Gx, detx = Q.greens_run(129, 2, True)
    eg, ed = Q.err_of(Gx, W.joined(x, key + 'G')), Q.err_of(detx, W.joined(x, key + 'det'), relative=True)
    print("recomputed: G %.3e det %.3e" % (eg, ed))
    assert eg <= 1e-14 and ed <= 1e-13


# ---- the header, the library, the walkers
def test_header_defines_the_bit_and_the_library_exports_the_bound():
    text = open(os.path.join(os.path.dirname(HERE), 'include', 'afqmc_hip.h')).read()
    assert re.search(r'^#define AFQ_THERMAL_QUAD\s+512\b', text, re.M)
    assert re.search(r'^int afq_thermal_quad_max_basis\(void\);', text, re.M)
    bits = [int(v) for v in re.findall(r'^#define AFQ_THERMAL_(?!EST_)\w+\s+(\d+)\b', text, re.M)]
    assert sorted(bits) == [1, 2, 4, 8, 16, 32, 128, 256, 512]                   # disjoint, and 64 stays the unknown bit
    others = L.THERMAL_FAR | L.THERMAL_WIDE | L.THERMAL_STREAMED_GREENS | L.THERMAL_DELAYED | 15 | 64
    assert L.THERMAL_QUAD == 512 and L.THERMAL_QUAD & others == 0
    assert int(L.load().afq_thermal_quad_max_basis()) == 256
    assert int(L.load().afq_thermal_far_max_basis()) == 128


def test_max_basis_has_a_quad_column_read_from_the_library():
    from pauxy_amd.walkers.thermal import MAX_BASIS
    M = int(L.load().afq_thermal_quad_max_basis())
    assert MAX_BASIS['planewave', 'quad'] == MAX_BASIS['hubbard_continuous', 'quad'] == M == 256
    assert MAX_BASIS['planewave', 'far'] == MAX_BASIS['hubbard_continuous', 'far'] == 128
    assert MAX_BASIS['planewave', 'wide'] == MAX_BASIS['hubbard_continuous', 'wide'] == 95
    assert (MAX_BASIS['planewave', False], MAX_BASIS['planewave', True]) == (47, 57)
    assert (MAX_BASIS['hubbard_continuous', False], MAX_BASIS['hubbard_continuous', True]) == (47, 63)
    assert MAX_BASIS['discrete', 'delayed'] == 128 and len(MAX_BASIS) == 11


def test_check_bound_words_the_quad_bound():
    from pauxy_amd.walkers.thermal import ThermalWalkers
    me = types.SimpleNamespace(wide_basis=False, streamed_greens=False, far_basis=False, quad_basis=True)
    for kind, unit in (('planewave', 'plane waves'), ('hubbard_continuous', 'sites')):
        for M in (64, 129, 147, 256):
            ThermalWalkers._check_bound(me, kind, M)
        with pytest.raises(NotImplementedError) as e:
            ThermalWalkers._check_bound(me, kind, 257)
        text = str(e.value)
        assert "M = 257 > 256 %s" % unit in text and "quad_basis" in text and "four columns" in text


class Qmc(object):
    dt, nstblz, nwalkers, ntot_walkers = 0.05, 5, 2, 2


def test_walkers_refuse_quad_basis_before_the_device():
    """On discrete fields by name; together with far_basis, wide_basis and streamed_greens; at M = 257 with the numbers."""
    from pauxy_amd.systems import UEG, Hubbard
    from pauxy_amd.trial_density import OneBody
    from pauxy_amd.walkers.handler import Walkers
    system = Hubbard(2, 2, 2, 2, 4.0, mu=1.0)
    trial = OneBody(system, 1.0, 0.05, options={'mu': 0.5})
    with pytest.raises(NotImplementedError, match='quad_basis belongs to the continuous fields'):
        Walkers(system, trial, Qmc(), walker_opts={'quad_basis': True})
    for other in ('far_basis', 'wide_basis', 'streamed_greens'):
        with pytest.raises(NotImplementedError, match='quad_basis and %s are two placements' % other):
            Walkers(system, trial, Qmc(), walker_opts={'quad_basis': True, other: True, 'continuous_fields': True})
    system = Hubbard(257, 1, 112, 112, 4.0, mu=1.0)
    trial = OneBody(system, 0.5, 0.05, options={'mu': 0.5})
    with pytest.raises(NotImplementedError, match='M = 257 > 256 sites.*four columns'):
        Walkers(system, trial, Qmc(), walker_opts={'quad_basis': True, 'continuous_fields': True})
    system = UEG(1.0, 2, 2, 8.0, full_lists=True)       # (the shell behind 251: ecut 7.5 is still 251 plane waves)
    system.mu = 0.245
    assert system.nbasis == 257
    with pytest.raises(NotImplementedError, match='M = %d > 256 plane waves.*four columns' % system.nbasis):
        Walkers(system, OneBody(system, 0.5, 0.05), Qmc(), walker_opts={'stack_size': 5, 'quad_basis': True})
