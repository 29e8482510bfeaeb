"""The delayed-update route of the real thermal walkers (AFQ_THERMAL_DELAYED, walkers: {delayed_updates: True}) on the
device: the wide real Green's function (thermal_greens_wide_kernel) and the delayed slice (thermal_slice_delayed_kernel)
against the extended-precision restatement under the rule of tests/test_gpu_thermal.py -- the device within
100 max(err_ref, 1e-15) of tests/thermal_ref_ext, err_ref the distance of the fp64 restatement of the delayed site loop
(tests/thermal_delayed_cases.DelayedPath) or of the reference's record from it; weights within M (slices so far) x that
bound; fields exactly, no decision of the restatement within 1e-9 of its threshold."""
import os

import numpy
import pytest

from pauxy_amd import _lib as L
from tests import thermal_delayed_cases as D
from tests import thermal_ref as tr
from tests import thermal_ref_ext as te
from tests.test_gpu_thermal import _Q, refused
from tests.test_gpu_thermal import check as _check
from tests.thermal_cases import Case

pytestmark = pytest.mark.gpu
BIT = L.THERMAL_DELAYED
NEW = {"thermal_slice_delayed_kernel", "thermal_greens_wide_kernel"}
OLD = {"thermal_slice_kernel", "thermal_greens_kernel"}


_MEASURED, _GROUP = [], [""]


def check(label, got, want64, want_ext, scale=1.0, factor=1.0):
    """The rule of tests/test_gpu_thermal.py, its figures kept for the precision table."""
    err_ref, err_dev = te.gerr(want64, want_ext) / scale, te.gerr(got, want_ext) / scale
    _MEASURED.append((_GROUP[0], label, err_ref, err_dev, factor * te.bound(err_ref)))
    _check(label, got, want64, want_ext, scale=scale, factor=factor)


@pytest.fixture(autouse=True)
def _group(request):
    _GROUP[0] = request.node.name
    yield


@pytest.fixture(scope="module", autouse=True)
def precision_table():
    """THERMAL_DELAYED_PRECISION_OUT=<file>: the worst fraction of the bound per test, as a markdown table."""
    yield
    out = os.environ.get("THERMAL_DELAYED_PRECISION_OUT")
    if not out or not _MEASURED:
        return
    worst = {}
    for group, label, err_ref, err_dev, bnd in _MEASURED:
        if group not in worst or err_dev / bnd > worst[group][2] / worst[group][3]:
            worst[group] = (label, err_ref, err_dev, bnd)
    lines = ["| test | worst comparison | err_ref | device | bound | fraction |", "|---|---|---|---|---|---|"]
    lines += ["| %s | %s | %.2e | %.2e | %.2e | %.3f |" % ((g,) + v + (v[2] / v[3],)) for g, v in worst.items()]
    lines += ["", "Largest fraction over every comparison of the module: %.3f." % max(e / b for _, _, _, e, b in _MEASURED), ""]
    with open(out, "w") as f:
        f.write("\n".join(lines))


def traced(dev):
    return set(dev.launch_trace_get())


# ---- 1: the wide real Green's function from an uploaded stack
def greens_case(case, nbins, stack_size, slice_ixs, nw=2, seed=5):
    Lts = nbins * stack_size
    stack = case.random_stack(nw, nbins, stack_size, seed)
    dev = D.delayed_device(case, nw, Lts, stack_size, stack_size)
    try:
        dev.set(L.F_THERMAL_STACK, stack)
        for slice_ix in slice_ixs:
            dev.thermal_greens(slice_ix)
            G = dev.get(L.F_THERMAL_G)
            order = tr.chain_order(slice_ix, stack_size, nbins)
            bins = [stack[:, b].reshape(nw * 2, case.M, case.M) for b in order]
            G64 = tr.strat_greens(bins).reshape(G.shape)
            Gx = te.strat_greens(bins).reshape(G.shape)
            check("G M=%d nbins=%d slice_ix=%d" % (case.M, nbins, slice_ix), G, G64, Gx)
    finally:
        dev.close()


@pytest.mark.parametrize("nbins", [1, 4])
@pytest.mark.parametrize("nx,ny", [(2, 2), (3, 2), (4, 4), (6, 6), (8, 8), (5, 13), (6, 11), (10, 10), (8, 16)])
def test_wide_real_greens_from_an_uploaded_stack(nx, ny, nbins):
    """M = 4, 6, 16, 36, 64 (the last of the one-column range), 65 (the first lane's second column), 66, 100 and 128
    (every lane's second column); one bin skips the chain loop."""
    greens_case(Case(nx, ny, 4.0, 0.05), nbins, 5, [0], nw=2 if nx * ny <= 66 else 1)


def test_wide_real_greens_every_starting_slice():
    greens_case(Case(3, 2, 4.0, 0.05), 4, 2, list(range(0, 9)))


def test_wide_real_greens_hardest_stack():
    """10 x 10, U = 8, four bins of 20 slices, one walker."""
    greens_case(Case(10, 10, 8.0, 0.05), 4, 20, [0, 40], nw=1)


# ---- 2: full paths slice by slice
PATHS = [
    # nx, ny, L, stack_size, nstblz, nw
    (3, 2, 10, 1, 1, 37),
    (3, 2, 10, 5, 5, 37),
    (3, 2, 10, 10, 5, 37),
    (4, 4, 10, 5, 5, 3),            # exactly one panel
    (4, 5, 10, 5, 5, 3),            # one panel and a ragged 4
    (8, 8, 10, 5, 5, 2),
    (5, 13, 10, 5, 5, 2),           # a ragged panel of 1
    (10, 10, 10, 5, 5, 1),
    (8, 16, 4, 2, 2, 2),
]


def walk_path(case, dev, p64, px, us, label=""):
    """One path on the device next to the two restatements, every slice under the rule."""
    M, Lts = case.M, len(us)
    check(label + "reset G", dev.get(L.F_THERMAL_G), p64.G, px.G)
    for ts in range(Lts):
        u = us[ts]
        f64 = p64.step(u)
        fx = px.step(u)
        fd = dev.thermal_propagate(u, 0.0, fetch_fields=True)
        assert px.min_margin > 1e-9 and p64.min_margin > 1e-9, (px.min_margin, p64.min_margin)
        numpy.testing.assert_array_equal(f64, fx)
        numpy.testing.assert_array_equal(fd, fx)
        assert dev.thermal_state() == (px.time_slice, px.block, px.counter, px.nbins)
        tag = label + "slice %d" % (ts + 1)
        err_ref = te.gerr(p64.G, px.G)
        check(tag + " G", dev.get(L.F_THERMAL_G), p64.G, px.G)
        sscale = max(1.0, float(numpy.max(numpy.abs(px.stack))))
        check(tag + " stack", dev.get(L.F_THERMAL_STACK), p64.stack, px.stack, scale=sscale)
        w = dev.get(L.F_WEIGHT)
        werr = float(numpy.max(numpy.abs(te.ext(w) / px.weight - 1)))
        wbnd = M * (ts + 1) * te.bound(err_ref)
        print("%s weight: device %.3e bound %.3e" % (tag, werr, wbnd))
        assert werr <= wbnd, (tag, werr, wbnd)


@pytest.mark.parametrize("nx,ny,Lts,stack_size,nstblz,nw", PATHS)
def test_full_path_against_the_extended_restatement(nx, ny, Lts, stack_size, nstblz, nw):
    case = Case(nx, ny, 4.0, 0.05, mu=1.0, mu_trial=0.8)
    rng = numpy.random.RandomState(100 * case.M + 10 * stack_size + nstblz)
    us = rng.random_sample((Lts, nw, case.M))
    p64, px = D.paths(case, Lts, stack_size, nstblz, nw)
    dev = D.delayed_device(case, nw, Lts, stack_size, nstblz)
    try:
        walk_path(case, dev, p64, px, us)
        E, nav = dev.thermal_energy()
        E64, nav64 = p64.energy(case.H1, case.U)
        Ex, navx = px.energy(case.H1, case.U)
        check("energy", E, E64, Ex, factor=case.h1_scale())
        check("nav", nav, nav64, navx, factor=case.h1_scale())
    finally:
        dev.close()


# ---- 3, 4: the recorded cases
def recorded_walker(d, pre, case, Lts, stack_size, nstblz, us, fields, weights, G_of, wscale=1.0):
    """One recorded walker through the library: the reference's fields exactly, G and weights by the rule, err_ref the
    larger of the record's and the restatement's distance."""
    M = case.M
    args = (case.BT, case.BH1, case.auxf, Lts, stack_size, nstblz, 1)
    p64 = D.DelayedPath(*args, BT_inv=case.BT_inv)
    px = te.path(*args, BT_inv=case.BT_inv)
    dev = D.delayed_device(case, 1, Lts, stack_size, nstblz)
    try:
        for ts in range(Lts):
            u = us[ts][None, :]
            p64.step(u)
            px.step(u)
            fd = dev.thermal_propagate(u, 0.0, fetch_fields=True)
            if wscale != 1.0:
                p64.weight, px.weight = p64.weight / wscale, px.weight / te.LD(wscale)
                dev.set(L.F_WEIGHT, dev.get(L.F_WEIGHT) / wscale)
            assert px.min_margin > 1e-9
            numpy.testing.assert_array_equal(fd[0], fields[ts])
            G = dev.get(L.F_THERMAL_G)
            check("%s slice %d G" % (pre, ts + 1), G, p64.G, px.G)
            if G_of(ts) is not None:
                check("%s slice %d G (record)" % (pre, ts + 1), G[0], G_of(ts), px.G[0])
            wbnd = M * (ts + 1) * te.bound(te.gerr(p64.G, px.G))
            werr = float(abs(te.ext(dev.get(L.F_WEIGHT)[0]) / px.weight[0] - 1))
            print("%s slice %d weight: device %.3e bound %.3e" % (pre, ts + 1, werr, wbnd))
            assert werr <= wbnd
            assert abs(dev.get(L.F_WEIGHT)[0] / weights[ts] - 1) <= 2 * wbnd
        return dev.thermal_energy(), p64, px
    finally:
        dev.close()


@pytest.mark.parametrize("k", [0, 1])
def test_the_4x4_reference_case_through_the_delayed_route(golden, k):
    """Case a of thermal_hubbard.npz (the genuine reference, stack_size 1 and 10) on a delayed handle."""
    d = golden("thermal_hubbard.npz")
    c = Case(4, 4, float(d['a_U']), float(d['a_dt']))
    c.BT, c.BT_inv, c.BH1, c.auxf = d['a_dmat'], d['a_dmat_inv'], d['a_BH1'], d['a_auxf']
    c.H1 = d['a_T']
    c.na, c.nb = [int(x) for x in d['a_nelec']]
    pre = 'a%d' % k
    (E, nav), p64, px = recorded_walker(d, pre, c, int(d['a_num_slices']), int(d['a_stack_sizes'][k]), int(d['a_nstblz']),
                                        d[pre + '_u'], d[pre + '_fields'], d[pre + '_weight'], lambda ts: d[pre + '_G'][ts],
                                        wscale=1.0e6)
    Ex, navx = px.energy(c.H1, c.U)
    E64, nav64 = p64.energy(c.H1, c.U)
    check("energy", E[0], E64[0], Ex[0], factor=c.h1_scale())
    check("nav", nav[0], nav64[0], navx[0], factor=c.h1_scale())


@pytest.mark.parametrize("name,tag", [("thermal_hubbard_large.npz", 'c'), ("thermal_hubbard_large_d.npz", 'd')])
def test_recorded_walker_beyond_64_sites_through_the_library(golden, name, tag):
    d = golden(name)
    assert float(d['min_margin']) > 1e-6
    c = D.FixtureCase(d, tag)
    keep = list(d[tag + '_G_slices'])
    (E, nav), p64, px = recorded_walker(d, tag, c, c.L, c.stack_size, c.nstblz, d[tag + '_u'], d[tag + '_fields'],
                                        d[tag + '_weight'],
                                        lambda ts: d[tag + '_G'][keep.index(ts + 1)] if ts + 1 in keep else None)
    Ex, navx = px.energy(c.H1, c.U)
    E64, nav64 = p64.energy(c.H1, c.U)
    check("energy", E[0], E64[0], Ex[0], factor=c.h1_scale())
    check("nav", nav[0], nav64[0], navx[0], factor=c.h1_scale())
    check("energy (record)", E[0], d[tag + '_energy'], Ex[0], factor=c.h1_scale())


@pytest.mark.parametrize("name,tag", [("thermal_hubbard_large.npz", 'c'), ("thermal_hubbard_large_d.npz", 'd')])
def test_recorded_walker_beyond_64_sites_through_the_python_classes(golden, monkeypatch, name, tag):
    from pauxy_amd.context import release_context
    from pauxy_amd.propagation.thermal_hubbard import ThermalDiscrete
    from pauxy_amd.systems import Hubbard
    from pauxy_amd.trial_density import OneBody
    from pauxy_amd.walkers.handler import Walkers
    d = golden(name)
    c = D.FixtureCase(d, tag)
    system = Hubbard(c.nx, c.ny, c.na, c.nb, c.U, mu=c.mu)
    trial = OneBody(system, float(d[tag + '_beta']), c.dt)
    assert abs(trial.mu - c.mu_trial) < 1e-12
    walk = Walkers(system, trial, _Q(dt=c.dt, nstblz=c.nstblz, nwalkers=1, ntot_walkers=1),
                   walker_opts={'stack_size': c.stack_size, 'low_rank': False, 'delayed_updates': True})
    try:
        prop = ThermalDiscrete(system, trial, _Q(dt=c.dt, nstblz=c.nstblz))
        stream = list(d[tag + '_u'].ravel())
        monkeypatch.setattr(numpy.random, 'random', lambda: stream.pop(0))
        p64 = D.DelayedPath(*c.args(), BT_inv=c.BT_inv)
        px = te.path(*c.args(), BT_inv=c.BT_inv)
        keep = list(d[tag + '_G_slices'])
        w = walk.walkers[0]
        walk.dev.launch_trace(True)
        for ts in range(c.L):
            p64.step(d[tag + '_u'][ts][None, :])
            px.step(d[tag + '_u'][ts][None, :])
            prop.propagate_walker(system, w, ts, 0)
            numpy.testing.assert_array_equal(prop.last_fields[0], d[tag + '_fields'][ts])
            check("%s slice %d G" % (tag, ts + 1), w.G, p64.G[0], px.G[0])
            if ts + 1 in keep:
                check("%s slice %d G (record)" % (tag, ts + 1), w.G, d[tag + '_G'][keep.index(ts + 1)], px.G[0])
            wbnd = c.M * (ts + 1) * te.bound(te.gerr(p64.G, px.G))
            assert abs(te.ext(w.weight) / px.weight[0] - 1) <= wbnd
            assert abs(w.weight / d[tag + '_weight'][ts] - 1) <= 2 * wbnd        # and the reference's own record
        assert not stream
        assert NEW <= traced(walk.dev) and not traced(walk.dev) & OLD
        assert te.gerr(numpy.array(w.local_energy(system)), d[tag + '_energy']) <= 2 * c.h1_scale() * te.bound(te.gerr(p64.G, px.G))
    finally:
        release_context(system, trial)


def test_recorded_driver_on_5x13_through_the_python_classes(golden):
    """Case e: ThermalAFQMC with delayed_updates over two paths from the reference's seed: its rows within 1e-9 (the
    tolerance the 4 x 4 driver is held to), the stream consumed as the reference consumed it (so the comb's parents,
    which the r of the stream decide, are the reference's)."""
    from pauxy_amd.context import release_context
    from pauxy_amd.qmc.thermal_afqmc import ThermalAFQMC
    d = golden("thermal_hubbard_large.npz")
    na, nb = [int(x) for x in d['e_nelec']]
    options = {'qmc': {'timestep': float(d['e_dt']), 'beta': float(d['e_beta']), 'num_walkers': int(d['e_nwalkers']),
                       'blocks': int(d['e_paths']), 'pop_control_freq': int(d['e_npop_control']),
                       'rng_seed': int(d['e_seed'])},
               'model': {'name': 'Hubbard', 'nx': int(d['e_nx']), 'ny': int(d['e_ny']), 'U': float(d['e_U']),
                         'mu': float(d['e_mu_system']), 'nup': na, 'ndown': nb},
               'trial': {'name': 'one_body'},
               'walkers': {'stack_size': int(d['e_stack_size']), 'delayed_updates': True},
               'estimates': {'mixed': {'verbose': False}}}
    # the restatement's run on the reference's matrices (case c's: the same lattice and trial) and stream: its combs
    c = D.FixtureCase(d, 'c')
    assert float(d['c_mu']) == float(d['e_mu'])
    nw = int(d['e_nwalkers'])
    p64 = D.DelayedPath(c.BT, c.BH1, c.auxf, c.L, c.stack_size, int(d['e_nstblz']), nw, BT_inv=c.BT_inv)
    want_parents, combs = [], p64.pop_control
    p64.pop_control = lambda r: want_parents.append(combs(r))
    rows64, used = p64.run(d['e_draws'], int(d['e_paths']), int(d['e_npop_control']), c.H1, c.U)
    assert used == len(d['e_draws']) and p64.min_margin > 1e-9 and len(want_parents) == len(d['e_r_pos'])
    state = numpy.random.get_state()
    afqmc = ThermalAFQMC(options=options)
    got_parents, inner = [], afqmc.walk.pop_control

    def pop_control(*a, **k):
        inner(*a, **k)
        got_parents.append(numpy.array(afqmc.walk.last_parent_ix))
    afqmc.walk.pop_control = pop_control
    try:
        assert afqmc.walk.delayed_updates and afqmc.qmc.nstblz == int(d['e_nstblz'])
        assert abs(afqmc.trial.mu - float(d['e_mu'])) < 1e-12
        afqmc.walk.dev.launch_trace(True)
        afqmc.run()
        assert NEW <= traced(afqmc.walk.dev) and not traced(afqmc.walk.dev) & OLD
        mixed = afqmc.estimators.estimators['mixed']
        assert mixed.header == list(d['e_header'])
        rows = numpy.array(mixed.blocks).real
        gold = d['e_blocks'].real
        assert rows.shape == gold.shape == (3, 12)
        scale = max(1.0, float(numpy.max(numpy.abs(gold[:, 1:11]))))
        err = float(numpy.max(numpy.abs(rows[:, :11] - gold[:, :11]))) / scale
        print("rows: %.3e (tolerance 1e-9)" % err)
        assert err <= 1e-9
        rs = numpy.random.RandomState(int(d['e_seed']))
        rs.random_sample(len(d['e_draws']))
        assert numpy.random.random() == rs.random_sample()
        assert len(got_parents) == len(want_parents) >= 1
        for a, b in zip(got_parents, want_parents):                 # the comb's parents, exactly
            numpy.testing.assert_array_equal(a, b)
        err64 = float(numpy.max(numpy.abs(rows64 - gold[:, 1:11]))) / scale
        print("restatement's rows against the record: %.3e" % err64)
        assert err64 <= 1e-9
    finally:
        numpy.random.set_state(state)
        release_context(afqmc.system, afqmc.trial)


# ---- 5: a zero-norm site
@pytest.mark.parametrize("site", [7, 19])
def test_zero_norm_site_inside_a_panel_and_at_the_ragged_end(site):
    """M = 20: site 7 sits in the middle of the first panel, site 19 is the last of the ragged one.  Walker 1's G has
    1 - G_ii = -4 there on both spins and nothing else in that row and column: both probabilities are clipped to zero,
    the weight is 0, the field -1, the factor zero -- G as the restatement, which skips the update, leaves it."""
    case = Case(4, 5, 4.0, 0.05)
    nw = 3
    p64, px = D.paths(case, 10, 5, 5, nw)
    dev = D.delayed_device(case, nw, 10, 5, 5)
    try:
        G = dev.get(L.F_THERMAL_G)
        G[1, :, site, :] = 0
        G[1, :, :, site] = 0
        G[1, :, site, site] = 5.0
        d = case.auxf - 1
        assert numpy.all(0.5 * (1 - 4.0 * d[:, 0]) * (1 - 4.0 * d[:, 1]) <= 0)
        dev.set(L.F_THERMAL_G, G)
        p64.G, px.G = G.copy(), te.ext(G)
        u = numpy.random.RandomState(site).random_sample((nw, case.M))
        f64, _ = p64.sites(u)
        fx, _ = px.sites(u)
        fd = dev.thermal_propagate(u, 0.0, fetch_fields=True)
        assert px.min_margin > 1e-9
        numpy.testing.assert_array_equal(fd, fx)
        numpy.testing.assert_array_equal(f64, fx)
        assert fd[1, site] == -1 and numpy.sum(fd == -1) == 1
        w = dev.get(L.F_WEIGHT)
        assert w[1] == 0.0 and w[0] > 0.0 and w[2] > 0.0
        assert abs(te.ext(w[0]) / px.weight[0] - 1) <= case.M * te.bound(te.gerr(p64.G, px.G))
        # (the slice ends with the wrap: both restatements apply it to the G the sites left)
        for p in (p64, px):
            p.G = p.BT[None] @ p.G @ p.BT_inv[None]
        check("G behind the dead site", dev.get(L.F_THERMAL_G), p64.G, px.G)
    finally:
        dev.close()


# ---- 6: the same bits
def test_reset_path_reset_and_another_grid_position_give_the_same_bits():
    case = Case(5, 13, 4.0, 0.05)
    Lts = 10
    us = numpy.random.RandomState(9).random_sample((Lts, 1, case.M))
    runs = []
    for nw, at in ((3, 0), (3, 0), (5, 4)):
        dev = D.delayed_device(case, nw, Lts, 5, 5)
        try:
            for _ in range(2 if not runs else 1):
                dev.thermal_reset()
                out = []
                for ts in range(Lts):
                    u = numpy.random.RandomState(100 + ts).random_sample((nw, case.M))
                    u[at] = us[ts, 0]
                    f = dev.thermal_propagate(u, 0.0, fetch_fields=True)
                    out.append((f[at], dev.get(L.F_THERMAL_G)[at], dev.get(L.F_THERMAL_STACK)[at], dev.get(L.F_WEIGHT)[at]))
                runs.append(out)
        finally:
            dev.close()
    assert len(runs) == 4
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            for x, y in zip(a, b):
                numpy.testing.assert_array_equal(x, y)


def test_comb_clones_at_65_sites_carry_green_function_and_stack():
    case = Case(5, 13, 4.0, 0.05)
    nw, Lts = 8, 10
    rng = numpy.random.RandomState(21)
    dev = D.delayed_device(case, nw, Lts, 5, 5)
    try:
        for ts in range(3):
            dev.thermal_propagate(rng.random_sample((nw, case.M)))
        wts = numpy.array([0.05, 2.6, 1.0, 0.1, 1.2, 0.02, 2.0, 1.03])
        dev.set(L.F_WEIGHT, wts)
        G0, S0 = dev.get(L.F_THERMAL_G), dev.get(L.F_THERMAL_STACK)
        mult, total = dev.popcontrol_comb(0.37, nw)
        want_mult, pairs = tr.comb_plan(wts / (wts.sum() / nw), 0.37, nw)
        numpy.testing.assert_array_equal(mult, want_mult)
        assert len(pairs) >= 2
        G1, S1 = G0.copy(), S0.copy()
        for c, k in pairs:
            G1[k], S1[k] = G0[c], S0[c]
        numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_G), G1)
        numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_STACK), S1)
        res = dev.thermal_estimates(one_rdm=True)
        assert res['one_rdm'].shape == (2, case.M, case.M) and numpy.all(numpy.isfinite(res['one_rdm']))
    finally:
        dev.close()


# ---- 7: the launch list
def test_launch_list_of_a_slice_with_and_without_a_rebuild():
    case = Case(5, 13, 4.0, 0.05)
    dev = D.delayed_device(case, 2, 10, 5, 5)
    try:
        rng = numpy.random.RandomState(3)
        dev.launch_trace(True)
        dev.thermal_propagate(rng.random_sample((2, case.M)))               # slice 1: no rebuild
        t = dev.launch_trace_get()
        assert {k: t[k][0] for k in t if k.startswith("thermal_")} == {"thermal_slice_delayed_kernel": 1, "thermal_wrap_kernel": 1}
        for _ in range(4):
            dev.thermal_propagate(rng.random_sample((2, case.M)))           # slice 5 rebuilds
        t = dev.launch_trace_get()
        assert {k: t[k][0] for k in t if k.startswith("thermal_")} == {
            "thermal_slice_delayed_kernel": 5, "thermal_wrap_kernel": 5, "thermal_greens_wide_kernel": 1}
    finally:
        dev.close()
    dev = Case(8, 8, 4.0, 0.05).device(2, 10, 5, 5)                        # without the bit: what it was
    try:
        dev.launch_trace(True)
        for _ in range(5):
            dev.thermal_propagate(numpy.random.RandomState(3).random_sample((2, 64)))
        t = dev.launch_trace_get()
        assert {k: t[k][0] for k in t if k.startswith("thermal_")} == {
            "thermal_slice_kernel": 5, "thermal_wrap_kernel": 5, "thermal_greens_kernel": 1}
    finally:
        dev.close()


def test_scratch_is_allocated_once():
    """The wide Green's function's scratch is the handle's, allocated by afq_thermal_configure: the handle's count of
    device allocations stands still over slices with and without a rebuild, afq_thermal_greens, afq_thermal_reset and a
    second path; a delayed handle holds exactly one block more than a handle of the same shape without the bit."""
    case = Case(5, 13, 4.0, 0.05)
    counts = {}
    for options in (0, BIT):
        dev = Case(8, 8, 4.0, 0.05).device(2, 10, 5, 5, options=options)
        try:
            counts[options] = dev.thermal_device_allocations()
        finally:
            dev.close()
    assert counts[BIT] == counts[0] + 1, counts
    dev = D.delayed_device(case, 3, 10, 5, 5)
    try:
        n0 = dev.thermal_device_allocations()
        assert n0 > 0
        rng = numpy.random.RandomState(4)
        for path in range(2):
            for ts in range(10):
                dev.thermal_propagate(rng.random_sample((3, case.M)))
                if ts == 6:
                    dev.thermal_greens(ts + 1)
            dev.thermal_reset()
            assert dev.thermal_device_allocations() == n0, (path, n0, dev.thermal_device_allocations())
    finally:
        dev.close()


# ---- 8: refusals
def test_refusals_around_the_bit():
    text = refused(lambda: D.delayed_device(Case(10, 13, 4.0, 0.05), 1, 10, 3, 3))       # (before stack_size is looked at)
    assert "M = 130 sites" in text and "128 columns" in text and "M <= 128" in text and "delayed_updates" in text
    assert "72" in refused(lambda: Case(9, 8, 4.0, 0.05).device(1, 10, 5, 5))            # without the bit: as before
    small = Case(2, 2, 4.0, 0.05)
    assert "unknown option bits" in refused(lambda: small.device(1, 10, 5, 5, options=64), L.AFQ_EINVAL)
    assert "unknown option bits" in refused(lambda: small.device(1, 10, 5, 5, options=64 | BIT), L.AFQ_EINVAL)
    assert "wide_basis" in refused(lambda: small.device(1, 10, 5, 5, options=L.THERMAL_WIDE | BIT), L.AFQ_EINVAL)
    assert "streamed_greens" in refused(lambda: small.device(1, 10, 5, 5, options=L.THERMAL_STREAMED_GREENS | BIT), L.AFQ_EINVAL)
    from tests import thermal_wide_cases as W
    from tests.test_gpu_thermal_wide import chain
    for fn in (lambda o: chain(9).device(2, 1, o), lambda o: W.ueg_case(7).device(1, 5, options=o)):
        text = refused(lambda: fn(BIT), L.AFQ_EINVAL)
        assert "delayed_updates belongs to the discrete fields" in text and "unknown" not in text
        assert "unknown option bits" in refused(lambda: fn(64), L.AFQ_EINVAL)
        assert "delayed_updates" in refused(lambda: fn(64 | BIT), L.AFQ_EINVAL)     # (named before the unknown bits)
    dev = D.delayed_device(small, 2, 10, 5, 5)
    try:
        text = refused(lambda: dev.thermal_estimates(average_gf=True))
        assert "average_gf" in text and "delayed_updates" in text
        dev.thermal_estimates(one_rdm=True)
    finally:
        dev.close()
