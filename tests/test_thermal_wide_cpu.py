"""The wide route of the complex thermal walkers (AFQ_THERMAL_WIDE, walkers: {wide_basis: True}) without a GPU: the
fp64 and the extended restatements replay the three fixtures recorded from the reference (thermal_ueg81.npz,
thermal_ueg93.npz, thermal_hubbard_cont_wide.npz) under the thermal tests' rule -- the fp64 restatement lies within
100 max(err_ref, 1e-15) of the extended one, err_ref the reference's own distance from it -- with the extended
results read from the stored files and their first slice recomputed here; the walkers' bounds and refusals around the
option before any device is touched; the header's bit and the library's bound."""
import os
import re
import types

import numpy
import pytest

from pauxy_amd import _lib as L
from tests import thermal_ueg_ref_ext as ue
from tests import thermal_wide_cases as W

HERE = os.path.dirname(os.path.abspath(__file__))


def held(label, got, ref, want_ext, relative=False):
    """`got` within bound(err_ref) of the extended result, err_ref the distance of `ref` (the reference's record)."""
    if relative:
        err_ref, err = ue.rerr(ref, want_ext), ue.rerr(got, want_ext)
    else:
        scale = max(1.0, float(numpy.max(numpy.abs(ue.ext(want_ext)))))
        err_ref, err = ue.gerr(ref, want_ext, scale), ue.gerr(got, want_ext, scale)
    print("%s: err_ref %.3e restatement %.3e bound %.3e" % (label, err_ref, err, ue.bound(err_ref)))
    assert err <= ue.bound(err_ref), (label, err_ref, err)
    assert err_ref <= 1e-10, (label, err_ref)                  # (the record and the restatement are the same path)


def replay(label, d, pre, r64, x, xpre, G_key):
    for q in W.SCALARS:
        for ts in range(len(r64[q])):
            held("%s slice %d %s" % (label, ts + 1, q), r64[q][ts], d[pre + q][ts], W.joined(x, xpre + q)[ts],
                 relative=q in ('M0', 'weight'))
    held(label + " " + G_key, r64[G_key], d[pre + G_key], W.joined(x, xpre + G_key))
    held(label + " M00", r64['M00'], d[pre + 'M00'], W.joined(x, xpre + 'M00'), relative=True)
    held(label + " energy", numpy.asarray(r64['energy']).real, d[pre + 'energy'].real, W.joined(x, xpre + 'energy').real)
    held(label + " nav", numpy.real(r64['nav']), complex(d[pre + 'nav']).real, W.joined(x, xpre + 'nav').real)
    assert r64['nclip'] == int(d[pre + 'nclip']) and r64['min_cos_margin'] > 1e-6


def first_slice_is_what_is_stored(label, rx, x, xpre):
    """One slice of the extended restatement recomputed: the stored numbers bit for bit (hi + lo)."""
    for q in W.SCALARS:
        hi, lo = W.split(rx[q][0])
        numpy.testing.assert_array_equal(hi, x[xpre + q + '_hi'][0], err_msg=label + q)
        numpy.testing.assert_array_equal(lo, x[xpre + q + '_lo'][0], err_msg=label + q)
    hi, lo = W.split(rx['M00'])
    numpy.testing.assert_array_equal(hi, x[xpre + 'M00_hi'])
    numpy.testing.assert_array_equal(lo, x[xpre + 'M00_lo'])


@pytest.mark.parametrize("name,pre,M,K", [W.UEG_A[0] + (81, None), W.UEG_A[1] + (93, None)])
def test_ueg_fixture_case_through_both_restatements(name, pre, M, K):
    d, x = W.golden(name), W.stored_ext()
    c = W.case_of_fixture(d, pre)
    assert c.M == M and c.L == 10 and int(d[pre + 'stack_size']) == 5 and list(d[pre + 'G_slices']) == [3, 10]
    assert d[pre + 'G'].shape == (2, 2, M, M) and d[pre + 'xi'].shape == (10, c.K)
    replay(pre, d, pre, W.ueg_run(name, pre, False), x, pre, 'G')
    first_slice_is_what_is_stored(pre, W.ueg_run(name, pre, True, nslice=1), x, pre)


@pytest.mark.parametrize("k,M", [(8, 64), (9, 65)])
def test_hubbard_fixture_case_through_both_restatements(k, M):
    d, x = W.golden(W.HUBBARD), W.stored_ext()
    pre, xpre = 'a%d_' % k, 'h%d_' % k
    assert int(d[pre + 'nx']) * int(d[pre + 'ny']) == M and int(d[pre + 'stack_size']) == 5
    assert pre + 'G' not in d and d[pre + 'G_last'].shape == (2, M, M)
    replay(pre, d, pre, W.hubbard_run(k, False), x, xpre, 'G_last')
    first_slice_is_what_is_stored(pre, W.hubbard_run(k, True, nslice=1), x, xpre)


def test_ueg_driver_at_81_against_the_stored_extended_run():
    """Case b5: the comb's parents of the reference and of the stored extended run are the same, a walker is cloned,
    and the reference's rows and weights lie within 1e-10 of the extended run's (a fp64 replay of the six walkers over
    two paths takes more than a minute here; the single-walker case above replays this basis slice by slice)."""
    name, k = W.UEG_B
    d, x = W.golden(name), W.stored_ext()
    pre = 'b%d_' % k
    assert int(d[pre + 'seed']) >= 8 and int(d[pre + 'nwalkers']) == 6 and numpy.any(d[pre + 'parent_ix'] > 1)
    numpy.testing.assert_array_equal(d[pre + 'parent_ix'], x[pre + 'parents'])
    wx, rx = W.joined(x, pre + 'wx'), W.joined(x, pre + 'rx')
    assert wx.shape == d[pre + 'weights'].shape == (20, 6) and rx.shape == (3, 10)
    assert ue.rerr(d[pre + 'weights'], wx) <= 1e-10
    assert ue.gerr(d[pre + 'blocks'].real[:, 1:11], rx, max(1.0, float(numpy.max(numpy.abs(rx))))) <= 1e-10


def test_hubbard_driver_on_8x8_through_the_fp64_restatement():
    d, x = W.golden(W.HUBBARD), W.stored_ext()
    pre = 'b%d_' % W.HUBBARD_B
    assert int(d[pre + 'nx']) == int(d[pre + 'ny']) == 8 and int(d[pre + 'nwalkers']) == 4
    rows, wts, parents, p = W.hubbard_driver(False)
    numpy.testing.assert_array_equal(numpy.array(parents), d[pre + 'parent_ix'])
    numpy.testing.assert_array_equal(numpy.array(parents), x['hb2_parents'])
    assert p.nclip == int(d[pre + 'nclip'])
    ref_w, wx = d[pre + 'weights'], W.joined(x, 'hb2_wx')
    alive = ref_w > 0
    assert numpy.all(numpy.asarray(wts)[~alive] == 0) and numpy.all(wx[~alive] == 0)
    held("b2 weights", numpy.asarray(wts)[alive], ref_w[alive], wx[alive], relative=True)
    cols = [0, 1, 2, 3, 4, 5, 6, 9]                    # (EHybrid is 0 and Overlap 1 in every row)
    held("b2 rows", numpy.asarray(rows)[:, cols], d[pre + 'blocks'].real[:, 1:11][:, cols], W.joined(x, 'hb2_rx')[:, cols],
         relative=True)


# ---- the header, the library, the walkers
def test_header_defines_the_bit_and_the_library_exports_the_bound():
    text = open(os.path.join(os.path.dirname(HERE), 'include', 'afqmc_hip.h')).read()
    assert re.search(r'^#define AFQ_THERMAL_WIDE\s+32\b', text, re.M)
    assert re.search(r'^int afq_thermal_wide_max_basis\(void\);', text, re.M)
    assert L.THERMAL_WIDE == 32 and L.THERMAL_WIDE & (L.THERMAL_STREAMED_GREENS | 15) == 0
    M = int(L.load().afq_thermal_wide_max_basis())
    lds = lambda m: 16 * (m * (m | 1) + 1152) + 512             # noqa: E731  (the header's formula)
    assert lds(M) <= 160 * 1024 < lds(M + 1) and M == 95 and lds(93) == 138384 + 18944


def test_max_basis_has_a_third_column_read_from_the_library():
    from pauxy_amd.walkers.thermal import MAX_BASIS
    M = int(L.load().afq_thermal_wide_max_basis())
    assert MAX_BASIS['planewave', 'wide'] == MAX_BASIS['hubbard_continuous', 'wide'] == M
    assert (MAX_BASIS['planewave', False], MAX_BASIS['planewave', True]) == (47, 57)
    assert (MAX_BASIS['hubbard_continuous', False], MAX_BASIS['hubbard_continuous', True]) == (47, 63)


def test_check_bound_words_the_wide_bound():
    from pauxy_amd.walkers.thermal import MAX_BASIS, ThermalWalkers
    me = types.SimpleNamespace(wide_basis=True, streamed_greens=False)
    top = MAX_BASIS['planewave', 'wide']
    for kind, unit in (('planewave', 'plane waves'), ('hubbard_continuous', 'sites')):
        for M in (64, 65, 81, 93, top):
            ThermalWalkers._check_bound(me, kind, M)
        with pytest.raises(NotImplementedError) as e:
            ThermalWalkers._check_bound(me, kind, top + 1)
        text = str(e.value)
        assert "M = %d > %d %s" % (top + 1, top, unit) in text and "wide_basis" in text and "one complex matrix" in text
    me = types.SimpleNamespace(wide_basis=False, streamed_greens=True)          # (the other columns speak as they did)
    with pytest.raises(NotImplementedError, match="M = 81 > 57 plane waves"):
        ThermalWalkers._check_bound(me, 'planewave', 81)


class Q(object):
    dt, nstblz, nwalkers, ntot_walkers = 0.05, 5, 2, 2


def test_walkers_refuse_wide_basis_before_the_device():
    """On discrete fields by name; together with streamed_greens; above the bound with the numbers."""
    from pauxy_amd.systems import UEG, Hubbard
    from pauxy_amd.trial_density import OneBody
    from pauxy_amd.walkers.handler import Walkers
    system = Hubbard(2, 2, 2, 2, 4.0, mu=1.0)
    trial = OneBody(system, 1.0, 0.05, options={'mu': 0.5})
    with pytest.raises(NotImplementedError, match='wide_basis belongs to the continuous fields'):
        Walkers(system, trial, Q(), walker_opts={'wide_basis': True})
    with pytest.raises(NotImplementedError, match='ask for one'):
        Walkers(system, trial, Q(), walker_opts={'wide_basis': True, 'streamed_greens': True, 'continuous_fields': True})
    system = UEG(1.0, 2, 2, 5.0, full_lists=True)
    system.mu = 0.245
    assert system.nbasis > 95
    with pytest.raises(NotImplementedError, match='M = %d > 95 plane waves' % system.nbasis):
        Walkers(system, OneBody(system, 0.5, 0.05), Q(), walker_opts={'stack_size': 5, 'wide_basis': True})
