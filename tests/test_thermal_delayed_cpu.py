"""The delayed-update route of the real thermal walkers (AFQ_THERMAL_DELAYED, walkers: {delayed_updates: True}) without
a GPU: the header's bit and the library's bound against its formula; the numpy restatement of the delayed site loop
(tests/thermal_delayed_cases.DelayedPath, the specification of thermal_slice_delayed_kernel) against the direct site
loop of tests/thermal_ref.Path; the fixture recorded from the reference beyond 64 sites against the fp64 and the
extended restatements under the thermal tests' rule; the walkers' refusals and acceptances before any device."""
import os
import re

import numpy
import pytest

from pauxy_amd import _lib as L
from tests import thermal_delayed_cases as D
from tests import thermal_ref as tr
from tests import thermal_ref_ext as te
from tests.thermal_cases import Case

HERE = os.path.dirname(os.path.abspath(__file__))


def held(label, got, ref, want_ext, scale=1.0):
    err_ref, err = te.gerr(ref, want_ext) / scale, te.gerr(got, want_ext) / scale
    print("%s: err_ref %.3e restatement %.3e bound %.3e" % (label, err_ref, err, te.bound(err_ref)))
    assert err <= te.bound(err_ref), (label, err_ref, err)


# ---- the header, the library, the walkers' table
def test_header_defines_the_bit_and_the_library_exports_the_bound():
    text = open(os.path.join(os.path.dirname(HERE), 'include', 'afqmc_hip.h')).read()
    assert re.search(r'^#define AFQ_THERMAL_DELAYED\s+128\b', text, re.M)
    assert re.search(r'^int afq_thermal_delayed_max_basis\(void\);', text, re.M)
    assert L.THERMAL_DELAYED == 128 and L.THERMAL_DELAYED & (L.THERMAL_WIDE | L.THERMAL_STREAMED_GREENS | 15 | 64) == 0
    assert L.SIGNATURES["afq_thermal_delayed_max_basis"] == []
    assert re.search(r'^int afq_thermal_device_allocations\(afq_handle \*h, int64_t \*out\);', text, re.M)
    assert int(L.load().afq_thermal_device_allocations(None, None)) == L.AFQ_EINVAL
    M = int(L.load().afq_thermal_delayed_max_basis())
    assert M == D.bound_by_formula() == D.DELAYED_MAX == 128
    # the issue's arithmetic: the Green's function at M = 128, the wrap at M = 128; every kernel within a work-group's LDS
    assert D.greens_wide_lds(128) == 141824 and D.wrap_lds(128) == 132096
    assert max(D.greens_wide_lds(M), D.slice_delayed_lds(M), D.wrap_lds(M)) <= D.LDS_MAX


def test_max_basis_has_the_delayed_key_read_from_the_library():
    from pauxy_amd.walkers.thermal import MAX_BASIS
    assert MAX_BASIS['discrete', 'delayed'] == int(L.load().afq_thermal_delayed_max_basis()) == 128
    assert MAX_BASIS['planewave', 'wide'] == 95                   # (the neighbours stay)


# ---- the delayed restatement against the direct one
@pytest.mark.parametrize("nx,ny", [(3, 3), (4, 4), (4, 5), (5, 13), (10, 10)])
def test_delayed_site_loop_is_the_direct_one_to_rounding(nx, ny):
    """M = 9, 16, 20, 65, 100 at KB = 1, 4, 16, M over the slices of one path (a rebuild and the wraps included): the
    fields of the direct loop exactly, G within the rule of the extended direct loop.  KB = 1 is the direct loop with
    the update as G + u w."""
    case = Case(nx, ny, 4.0, 0.05, mu=1.0, mu_trial=0.8)
    M, nw, Lts = case.M, 2, 4 if nx * ny > 64 else 6
    args = (case.BT, case.BH1, case.auxf, Lts, 2, 2, nw)
    p64 = tr.Path(*args, BT_inv=case.BT_inv)
    px = te.path(*args, BT_inv=case.BT_inv)
    pd = [D.DelayedPath(*args, BT_inv=case.BT_inv, KB=kb) for kb in (1, 4, 16, M)]
    rng = numpy.random.RandomState(11 + M)
    for ts in range(Lts):
        u = rng.random_sample((nw, M))
        f64, fx = p64.step(u), px.step(u)
        assert px.min_margin > 1e-9
        numpy.testing.assert_array_equal(f64, fx)
        for p in pd:
            numpy.testing.assert_array_equal(p.step(u), fx)
            assert p.min_margin > 1e-9
            held("M=%d KB=%d slice %d G" % (M, p.kb_max, ts + 1), p.G, p64.G, px.G)
            sscale = max(1.0, float(numpy.max(numpy.abs(px.stack))))
            held("M=%d KB=%d slice %d stack" % (M, p.kb_max, ts + 1), p.stack, p64.stack, px.stack, scale=sscale)
            assert te.gerr(p.weight / px.weight, 1.0) <= M * (ts + 1) * te.bound(te.gerr(p64.G, px.G))


def test_delayed_site_loop_skips_a_zero_norm_site():
    """A walker whose probabilities both vanish at one site: weight 0, field -1, a zero factor -- G as the direct loop
    leaves it, the other walker untouched."""
    case = Case(4, 5, 4.0, 0.05)
    args = (case.BT, case.BH1, case.auxf, 10, 5, 5, 2)
    p64, pd = tr.Path(*args, BT_inv=case.BT_inv), D.DelayedPath(*args, BT_inv=case.BT_inv)
    G0 = pd.G.copy()
    for site in (7, 19):                                          # the middle of a panel; the last of the ragged one
        G = G0.copy()
        G[1, :, site, :] = 0
        G[1, :, :, site] = 0
        G[1, :, site, site] = 5.0
        p64.G, pd.G = G.copy(), G.copy()
        p64.weight, pd.weight = numpy.ones(2), numpy.ones(2)
        u = numpy.random.RandomState(site).random_sample((2, case.M))
        fa, _ = p64.sites(u)
        fb, _ = pd.sites(u)
        numpy.testing.assert_array_equal(fa, fb)
        assert fb[1, site] == -1 and numpy.sum(fb == -1) == 1 and pd.weight[1] == 0.0 and pd.weight[0] > 0
        assert te.gerr(pd.G, p64.G) <= 1e-13


# ---- the fixture
def load(name):
    return numpy.load(os.path.join(HERE, 'golden', name))


def fixture_paths(d, tag, kb=D.KB):
    c = D.FixtureCase(d, tag)
    return c, tr.Path(*c.args(), BT_inv=c.BT_inv), D.DelayedPath(*c.args(), BT_inv=c.BT_inv, KB=kb), \
        te.path(*c.args(), BT_inv=c.BT_inv)


@pytest.mark.parametrize("name,tag,M,keep", [("thermal_hubbard_large.npz", 'c', 65, [1, 5, 10]),
                                             ("thermal_hubbard_large_d.npz", 'd', 100, [5, 10])])
def test_fixture_walker_through_the_restatements(name, tag, M, keep):
    """Cases c and d as test_thermal_cpu.py holds case a: the reference's fields from the direct and the delayed
    restatement exactly, its G, weights, energies and nav within the rule of the extended restatement."""
    d = load(name)
    assert float(d['min_margin']) > 1e-6 and list(d[tag + '_G_slices']) == keep
    c, p64, pd, px = fixture_paths(d, tag)
    Lts = c.L
    assert c.M == M and Lts == 10 and c.stack_size == 5 and d[tag + '_G'].shape == (len(keep), 2, M, M)
    for ts in range(Lts):
        u = d[tag + '_u'][ts][None, :]
        for p in (p64, pd, px):
            numpy.testing.assert_array_equal(p.step(u)[0], d[tag + '_fields'][ts])
        assert px.min_margin > 1e-9 and pd.min_margin > 1e-9
        if ts + 1 in keep:
            Gref = d[tag + '_G'][keep.index(ts + 1)]
            held("%s slice %d G direct" % (tag, ts + 1), p64.G[0], Gref, px.G[0])
            held("%s slice %d G delayed" % (tag, ts + 1), pd.G[0], Gref, px.G[0])
        wbnd = M * (ts + 1) * te.bound(te.gerr(p64.G, px.G))
        for p in (p64, pd):
            assert abs(te.ext(p.weight[0]) / px.weight[0] - 1) <= wbnd
        assert abs(te.ext(d[tag + '_weight'][ts]) / px.weight[0] - 1) <= wbnd
    T, U, scale = c.H1, c.U, c.h1_scale()
    Ex, navx = px.energy(T, U)
    for p in (p64, pd):
        E, nav = p.energy(T, U)
        assert te.gerr(E[0], Ex[0]) <= scale * te.bound(te.gerr(p64.G, px.G))
        assert te.gerr(nav[0], navx[0]) <= scale * te.bound(te.gerr(p64.G, px.G))
    assert te.gerr(d[tag + '_energy'], Ex[0]) <= scale * te.bound(te.gerr(p64.G, px.G))
    assert te.gerr(float(d[tag + '_nav']), navx[0]) <= scale * te.bound(te.gerr(p64.G, px.G))


def test_fixture_driver_record_is_whole():
    """Case e: 4 walkers on 5 x 13 over two paths: every site uniform and every comb's r in the stream, three rows."""
    d = load("thermal_hubbard_large.npz")
    M, nw, Lts, paths = 65, int(d['e_nwalkers']), int(d['e_ntime_slices']), int(d['e_paths'])
    assert int(d['e_nx']) * int(d['e_ny']) == M and nw == 4 and Lts == 10 and int(d['e_stack_size']) == 5
    assert len(d['e_draws']) == paths * Lts * nw * M + len(d['e_r_pos']) and len(d['e_r_pos']) >= 1
    assert d['e_blocks'].shape == (3, 12) and int(d['e_npop_control']) == 5
    # the comb's r sit behind whole slices of site uniforms
    for k, pos in enumerate(d['e_r_pos']):
        assert (int(pos) - k) % (nw * M) == 0


# ---- the walkers, before the device
class Q(object):
    dt, nstblz, nwalkers, ntot_walkers = 0.05, 5, 2, 2


def test_walkers_take_and_refuse_delayed_updates_before_the_device(monkeypatch):
    from pauxy_amd.systems import UEG, Hubbard
    from pauxy_amd.trial_density import OneBody
    from pauxy_amd.walkers import thermal as wt
    from pauxy_amd.walkers.handler import Walkers

    class NoDevice(object):
        """Stands where the context's device would: the refusals and the acceptance below come before it is used."""
        def __getattr__(self, name):
            if name == 'walkers_alloc':
                return lambda n: None
            raise AssertionError("the device was touched: " + name)
    monkeypatch.setattr(wt, 'get_context', lambda *a, **k: type('Ctx', (), {'dev': NoDevice()})())
    # 72 sites: refused without the key as before (with a hint now), taken with it
    system = Hubbard(9, 8, 30, 30, 4.0, mu=1.0)
    trial = OneBody(system, 0.5, 0.05, options={'mu': 0.5})
    with pytest.raises(NotImplementedError, match=r"M = 72 > 64 sites is not supported.*delayed_updates") as e:
        Walkers(system, trial, Q(), walker_opts={'stack_size': 5})
    assert "128" in str(e.value)
    walk = Walkers(system, trial, Q(), walker_opts={'stack_size': 5, 'delayed_updates': True})
    assert walk.delayed_updates and walk.kind == 'discrete' and walk.stack_size == 5
    # above the bound with the numbers
    system = Hubbard(10, 13, 60, 60, 4.0, mu=1.0)
    with pytest.raises(NotImplementedError, match="M = 130 > 128 sites is not supported with delayed_updates"):
        Walkers(system, OneBody(system, 0.5, 0.05, options={'mu': 0.5}), Q(), walker_opts={'delayed_updates': True})
    # by name on the complex kinds
    system = Hubbard(2, 2, 2, 2, 4.0, mu=1.0)
    trial = OneBody(system, 1.0, 0.05, options={'mu': 0.5})
    with pytest.raises(NotImplementedError, match='delayed_updates belongs to the discrete fields'):
        Walkers(system, trial, Q(), walker_opts={'delayed_updates': True, 'continuous_fields': True})
    system = UEG(1.0, 2, 2, 1.0, full_lists=True)
    system.mu = 0.245
    with pytest.raises(NotImplementedError, match='delayed_updates belongs to the discrete fields'):
        Walkers(system, OneBody(system, 0.5, 0.05), Q(), walker_opts={'stack_size': 5, 'delayed_updates': True})
    # the neighbours speak as they did
    system = Hubbard(2, 2, 2, 2, 4.0, mu=1.0)
    with pytest.raises(NotImplementedError, match='wide_basis belongs to the continuous fields'):
        Walkers(system, trial, Q(), walker_opts={'wide_basis': True})


def test_mixed_estimator_refuses_average_gf_on_a_delayed_population():
    import types
    from pauxy_amd.estimators.mixed import Mixed

    class Psi(object):
        delayed_updates = True

        def ensure_configured(self):
            raise AssertionError("the device was configured before the refusal")
    me = types.SimpleNamespace(average_gf=True, calc_one_rdm=False, structure_factor=False, names=None, estimates=None)
    with pytest.raises(NotImplementedError, match="average_gf is not supported on a population with delayed_updates"):
        Mixed.update_thermal_sweep(me, Psi())
