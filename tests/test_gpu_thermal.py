"""Thermal (finite-temperature) Hubbard walkers on the device against the extended-precision restatement
(tests/thermal_ref_ext.py) under the project's accuracy rule: the device lies within 100 max(err_ref, 1e-15) of the
extended result, err_ref the fp64 restatement's own distance from it on the same fields.  Every comparison prints its
three figures (err_ref, device error, bound)."""
import numpy
import pytest

from pauxy_amd import _lib as L
from tests import thermal_ref as tr
from tests import thermal_ref_ext as te
from tests.thermal_cases import Case

pytestmark = pytest.mark.gpu


def check(label, got, want64, want_ext, scale=1.0, factor=1.0):
    """device within factor x bound(err_ref) of the extended result, both errors on the scale `scale`."""
    err_ref = te.gerr(want64, want_ext) / scale
    err_dev = te.gerr(got, want_ext) / scale
    bnd = factor * te.bound(err_ref)
    print("%s: err_ref %.3e device %.3e bound %.3e" % (label, err_ref, err_dev, bnd))
    assert numpy.all(numpy.isfinite(got)), label
    assert err_dev <= bnd, (label, err_ref, err_dev, bnd)


def greens_case(case, nbins, stack_size, slice_ixs, nw=2, seed=5):
    Lts = nbins * stack_size
    stack = case.random_stack(nw, nbins, stack_size, seed)
    dev = case.device(nw, Lts, stack_size, stack_size)
    try:
        dev.set(L.F_THERMAL_STACK, stack)
        numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_STACK), stack)
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


@pytest.mark.parametrize("nbins", [1, 4, 8])
@pytest.mark.parametrize("nx,ny", [(2, 2), (3, 2), (4, 4), (6, 6), (8, 8)])
def test_stratified_greens_from_an_uploaded_stack(nx, ny, nbins):
    """M = 4, 6 (below one tile, not a multiple of 4), 16 (one tile), 36 (padded tiles), 64 (the largest); one bin skips
    the chain loop."""
    greens_case(Case(nx, ny, 4.0, 0.05), nbins, 5, [0])


def test_stratified_greens_every_starting_slice():
    """Every slice_ix of one case, the final one (bin_ix == nbins -> the chain starts at bin 0) included."""
    greens_case(Case(3, 2, 4.0, 0.05), 4, 2, list(range(0, 9)))


def test_stratified_greens_hardest_stack():
    """8 x 8, U = 8, beta = 4 as 4 bins of 20 slices: bins of condition 1e8."""
    greens_case(Case(8, 8, 8.0, 0.05), 4, 20, [0, 40], nw=1)


PATHS = [
    # nx, ny, L, stack_size, nstblz, nw
    (3, 2, 10, 1, 1, 37),
    (3, 2, 10, 1, 5, 5),
    (3, 2, 10, 5, 1, 1),
    (3, 2, 10, 5, 5, 37),
    (3, 2, 10, 10, 1, 5),
    (3, 2, 10, 10, 5, 1),
    (3, 3, 10, 5, 5, 5),
    (8, 8, 10, 5, 5, 5),
]


@pytest.mark.parametrize("nx,ny,Lts,stack_size,nstblz,nw", PATHS)
def test_full_path_against_the_extended_restatement(nx, ny, Lts, stack_size, nstblz, nw):
    """G, stack, fields and weight after every slice of one path; the uniforms are the test's."""
    case = Case(nx, ny, 4.0, 0.05, mu=1.0, mu_trial=0.8)
    M = case.M
    rng = numpy.random.RandomState(100 * M + 10 * stack_size + nstblz)
    p64 = tr.Path(case.BT, case.BH1, case.auxf, Lts, stack_size, nstblz, nw, BT_inv=case.BT_inv)
    px = te.path(case.BT, case.BH1, case.auxf, Lts, stack_size, nstblz, nw, BT_inv=case.BT_inv)
    dev = case.device(nw, Lts, stack_size, nstblz)
    try:
        check("reset G", dev.get(L.F_THERMAL_G), p64.G, px.G)
        for ts in range(Lts):
            u = rng.random_sample((nw, M))
            f64 = p64.step(u)
            fx = px.step(u)
            fd = dev.thermal_propagate(u, 0.0, fetch_fields=True)
            assert px.min_margin > 1e-9, px.min_margin      # no decision within rounding of its threshold
            numpy.testing.assert_array_equal(f64, fx)
            numpy.testing.assert_array_equal(fd, fx)
            assert dev.thermal_state() == (px.time_slice, px.block, px.counter, px.nbins)
            tag = "slice %d" % (ts + 1)
            G = dev.get(L.F_THERMAL_G)
            err_ref = te.gerr(p64.G, px.G)
            check(tag + " G", G, p64.G, px.G)
            sscale = max(1.0, float(numpy.max(numpy.abs(px.stack))))
            check(tag + " stack", dev.get(L.F_THERMAL_STACK), p64.stack, px.stack, scale=sscale)
            w = dev.get(L.F_WEIGHT)
            wx = px.weight
            werr = float(numpy.max(numpy.abs(te.ext(w) / wx - 1)))
            wbnd = M * (ts + 1) * te.bound(err_ref)
            print("%s weight: device %.3e bound %.3e" % (tag, werr, wbnd))
            assert werr <= wbnd, (tag, werr, wbnd)
        E, nav = dev.thermal_energy()
        E64, nav64 = p64.energy(case.H1, case.U)
        Ex, navx = px.energy(case.H1, case.U)
        check("energy", E, E64, Ex, factor=case.h1_scale())
        check("nav", nav, nav64, navx, factor=case.h1_scale())
    finally:
        dev.close()


def test_reset_path_reset_reproduces_the_path_bit_for_bit():
    case = Case(3, 3, 4.0, 0.05)
    nw, Lts = 5, 10
    us = numpy.random.RandomState(9).random_sample((Lts, nw, case.M))
    dev = case.device(nw, Lts, 5, 5)
    try:
        runs = []
        for _ in range(2):
            dev.thermal_reset()
            assert dev.thermal_state() == (0, 0, 0, 2)
            numpy.testing.assert_array_equal(dev.get(L.F_WEIGHT), numpy.ones(nw))
            out = []
            for ts in range(Lts):
                f = dev.thermal_propagate(us[ts], 0.0, fetch_fields=True)
                out.append((f, dev.get(L.F_THERMAL_G), dev.get(L.F_THERMAL_STACK), dev.get(L.F_WEIGHT)))
            runs.append(out)
            with pytest.raises(L.AfqError) as e:          # the path is complete
                dev.thermal_propagate(us[0])
            assert e.value.code == L.AFQ_ESTATE
        for a, b in zip(*runs):
            for x, y in zip(a, b):
                numpy.testing.assert_array_equal(x, y)
    finally:
        dev.close()


def test_comb_clones_carry_green_function_and_stack():
    case = Case(3, 2, 4.0, 0.05)
    nw, Lts = 8, 10
    rng = numpy.random.RandomState(21)
    dev = case.device(nw, Lts, 5, 5)
    try:
        for ts in range(3):
            dev.thermal_propagate(rng.random_sample((nw, case.M)))
        wts = numpy.array([0.05, 2.6, 1.0, 0.1, 1.2, 0.02, 2.0, 1.03])
        dev.set(L.F_WEIGHT, wts)
        G0, S0 = dev.get(L.F_THERMAL_G), dev.get(L.F_THERMAL_STACK)
        mult, total = dev.popcontrol_comb(0.37, nw)
        assert abs(total - wts.sum()) < 1e-12
        want_mult, pairs = tr.comb_plan(wts / (wts.sum() / nw), 0.37, nw)
        numpy.testing.assert_array_equal(mult, want_mult)
        assert len(pairs) >= 2
        G1, S1 = G0.copy(), S0.copy()
        for c, k in pairs:
            G1[k], S1[k] = G0[c], S0[c]
        numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_G), G1)
        numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_STACK), S1)
        numpy.testing.assert_array_equal(dev.get(L.F_WEIGHT), numpy.ones(nw))
        # the cap of the thermal driver: |w| > 0.1 total -> 0.1 total, total the comb's
        dev.set(L.F_WEIGHT, numpy.array([0.5, 3.0, 0.7, 1.0, 1.0, 1.0, 0.2, 0.6]))
        dev.cap_weights(0.1, -1.0)
        cap = 0.1 * wts.sum()
        numpy.testing.assert_allclose(dev.get(L.F_WEIGHT), numpy.minimum([0.5, 3.0, 0.7, 1.0, 1.0, 1.0, 0.2, 0.6], cap),
                                      rtol=1e-15)
    finally:
        dev.close()


def test_zero_norm_site_kills_the_walker_and_leaves_g_alone():
    """A G for which both probabilities of every site are negative and clipped to zero: weight 0, field -1."""
    case = Case(2, 2, 4.0, 0.05)
    dev = case.device(2, 10, 5, 5)
    try:
        G = dev.get(L.F_THERMAL_G)
        # 1 - G_ii = -4 on both spins: field 0 turns the up factor negative (delta[0, up] > 0), field 1 the down factor
        G[1, 0] = numpy.eye(4) * 5.0
        G[1, 1] = numpy.eye(4) * 5.0
        d = case.auxf - 1
        probs = 0.5 * (1 - 4.0 * d[:, 0]) * (1 - 4.0 * d[:, 1])
        assert numpy.all(probs <= 0), probs
        dev.set(L.F_THERMAL_G, G)
        f = dev.thermal_propagate(numpy.full((2, 4), 0.5), fetch_fields=True)
        assert numpy.all(f[1] == -1) and numpy.all(f[0] >= 0)
        w = dev.get(L.F_WEIGHT)
        assert w[1] == 0.0 and w[0] > 0.0
    finally:
        dev.close()


# ---- refusals, each by name
def refused(fn, code=None):
    with pytest.raises(L.AfqError) as e:
        fn()
    assert e.value.code == (L.AFQ_EUNSUPPORTED if code is None else code), e.value
    return str(e.value)


def test_m_72_is_refused():
    assert "72" in refused(lambda: Case(9, 8, 4.0, 0.05).device(1, 10, 5, 5))


@pytest.mark.parametrize("bit,word", [(L.THERMAL_CHARGE, "charge_decomposition"), (L.THERMAL_FREE_PROJECTION, "free_projection"),
                                      (L.THERMAL_LOW_RANK, "low_rank"), (L.THERMAL_AVERAGE_GF, "average_gf")])
def test_option_is_refused(bit, word):
    assert word in refused(lambda: Case(2, 2, 4.0, 0.05).device(1, 10, 5, 5, options=bit))


def test_windows_rdm_and_pair_branch_are_refused_on_a_thermal_handle():
    dev = Case(2, 2, 4.0, 0.05).device(4, 10, 5, 5)
    try:
        assert "back-propagation" in refused(lambda: dev.bp_configure(4))
        assert "ITCF" in refused(lambda: dev.itcf_configure(2))
        assert "rdm" in refused(lambda: dev.estimates_rdm(True))
        assert "pair_branch" in refused(lambda: dev.popcontrol_pair_branch(numpy.full(2, 0.5), 4, 0.1, 4.0))
    finally:
        dev.close()


def test_other_systems_and_bad_stack_size_are_refused():
    from pauxy_amd.device import AfqDevice
    from pauxy_amd.systems import synthetic_generic
    from pauxy_amd.trial import rhf_trial_generic
    sysg = synthetic_generic(6, 8, (2, 2), seed=3)
    trial = rhf_trial_generic(sysg)
    dev = AfqDevice(0)
    try:
        dev.set_system_generic(sysg.hs_pot, trial._rchol, sysg.H1.astype(complex), sysg.ecore, 2, 2)
        dev.walkers_alloc(2)
        eye = numpy.array([numpy.eye(6)] * 2)
        assert "Hubbard" in refused(lambda: dev.thermal_configure(10, 5, 5, eye, eye, eye, numpy.ones((2, 2))))
    finally:
        dev.close()
    case = Case(2, 2, 4.0, 0.05)
    refused(lambda: case.device(1, 10, 3, 3), L.AFQ_EINVAL)        # stack_size does not divide the slices
    dev = AfqDevice(0)
    try:
        refused(lambda: dev.thermal_reset(), L.AFQ_ESTATE)         # not configured
    finally:
        dev.close()


# ---- the cases recorded from the genuine reference, through the Python classes
class _Q(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.mark.parametrize("k", [0, 1])
def test_golden_walker_through_the_python_classes(golden, monkeypatch, k):
    """Case (a): one walker at stack_size 1 and 10 with the recorded uniforms fed through numpy.random.random: the
    fields of the reference exactly, G and the weight under the rule after every slice, the final energies and nav."""
    from pauxy_amd.context import release_context
    from pauxy_amd.propagation.thermal_hubbard import ThermalDiscrete
    from pauxy_amd.systems import Hubbard
    from pauxy_amd.trial_density import OneBody
    from pauxy_amd.walkers.handler import Walkers
    d = golden("thermal_hubbard.npz")
    assert float(d['min_margin']) > 1e-6
    ss, Lts, M = int(d['a_stack_sizes'][k]), int(d['a_num_slices']), 16
    na, nb = [int(x) for x in d['a_nelec']]
    system = Hubbard(4, 4, na, nb, float(d['a_U']), mu=float(d['a_mu_system']))
    trial = OneBody(system, float(d['a_beta']), float(d['a_dt']))
    walk = Walkers(system, trial, _Q(dt=float(d['a_dt']), nstblz=10, nwalkers=1, ntot_walkers=1),
                   walker_opts={'stack_size': ss, 'low_rank': False})
    try:
        assert walk.walker_type == 'thermal' and walk.stack_size == ss
        prop = ThermalDiscrete(system, trial, _Q(dt=float(d['a_dt']), nstblz=int(d['a_nstblz'])))
        stream = list(d['a%d_u' % k].ravel())
        monkeypatch.setattr(numpy.random, 'random', lambda: stream.pop(0))
        args = (d['a_dmat'], d['a_BH1'], d['a_auxf'], Lts, ss, int(d['a_nstblz']), 1)
        p64 = tr.Path(*args, BT_inv=d['a_dmat_inv'])
        px = te.path(*args, BT_inv=d['a_dmat_inv'])
        w = walk.walkers[0]
        check("trial G", w.G, p64.G[0], px.G[0])
        for ts in range(Lts):
            u = d['a%d_u' % k][ts][None, :]
            p64.step(u)
            px.step(u)
            p64.weight, px.weight = p64.weight / 1.0e6, px.weight / te.LD(1.0e6)
            prop.propagate_walker(system, w, ts, 0)
            w.weight = w.weight / 1.0e6
            numpy.testing.assert_array_equal(prop.last_fields[0], d['a%d_fields' % k][ts])
            err_ref = te.gerr(p64.G, px.G)
            check("slice %d G" % (ts + 1), w.G, p64.G[0], px.G[0])
            werr = float(abs(te.ext(w.weight) / px.weight[0] - 1))
            wbnd = M * (ts + 1) * te.bound(err_ref)
            print("slice %d weight: device %.3e bound %.3e" % (ts + 1, werr, wbnd))
            assert werr <= wbnd
            assert abs(w.weight / d['a%d_weight' % k][ts] - 1) <= 2 * wbnd        # and the reference's own record
        assert not stream
        E64, nav64 = p64.energy(d['a_T'], float(d['a_U']))
        Ex, navx = px.energy(d['a_T'], float(d['a_U']))
        scale = float(numpy.max(numpy.sum(numpy.abs(d['a_T'][0]), axis=0))) + float(d['a_U']) * M
        E, nav = walk.dev.thermal_energy()
        check("energy", E[0], E64[0], Ex[0], factor=scale)
        check("nav", nav[0], nav64[0], navx[0], factor=scale)
        assert te.gerr(numpy.array(w.local_energy(system)), d['a%d_energy' % k]) <= 2 * scale * te.bound(te.gerr(p64.G, px.G))
    finally:
        release_context(system, trial)


def test_golden_driver_through_the_python_classes(golden):
    """Case (b): ThermalAFQMC with 6 walkers over two paths -- comb events, the weight cap, the reset between paths, the
    Nav column -- from the same seed as the reference's run: its estimator rows."""
    from pauxy_amd.context import release_context
    from pauxy_amd.qmc.thermal_afqmc import ThermalAFQMC
    d = golden("thermal_hubbard.npz")
    options = {'qmc': {'timestep': float(d['b_dt']), 'beta': float(d['b_beta']), 'num_walkers': int(d['b_nwalkers']),
                       'blocks': int(d['b_paths']), 'pop_control_freq': int(d['b_npop_control']),
                       'rng_seed': int(d['b_seed'])},
               'model': {'name': 'Hubbard', 'nx': 4, 'ny': 4, 'U': 4, 'mu': 1.0, 'nup': 7, 'ndown': 7},
               'trial': {'name': 'one_body'},
               'walkers': {'stack_size': int(d['b_stack_size'])},
               'estimates': {'mixed': {'verbose': False}}}
    state = numpy.random.get_state()
    afqmc = ThermalAFQMC(options=options)
    try:
        assert afqmc.qmc.nstblz == int(d['b_nstblz']) and afqmc.qmc.ntime_slices == int(d['b_ntime_slices'])
        assert abs(afqmc.trial.mu - float(d['b_mu'])) < 1e-12
        afqmc.run()
        mixed = afqmc.estimators.estimators['mixed']
        assert mixed.header == list(d['b_header'])
        rows = numpy.array(mixed.blocks).real
        gold = d['blocks'].real
        assert rows.shape == gold.shape == (3, 12)
        scale = max(1.0, float(numpy.max(numpy.abs(gold[:, 1:11]))))
        err = float(numpy.max(numpy.abs(rows[:, :11] - gold[:, :11]))) / scale
        print("rows: %.3e (tolerance 1e-9)" % err)
        assert err <= 1e-9
        # the stream was consumed exactly as the reference consumed it: the next uniform is the next of seed 7
        rs = numpy.random.RandomState(int(d['b_seed']))
        rs.random_sample(len(d['b_draws']))
        assert numpy.random.random() == rs.random_sample()
        assert afqmc.walk.last_parent_ix is not None
    finally:
        numpy.random.set_state(state)
        release_context(afqmc.system, afqmc.trial)
