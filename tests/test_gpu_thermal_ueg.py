"""Thermal (finite-temperature) walkers of the uniform electron gas with continuous fields on the device, against the
extended-precision restatement (tests/thermal_ueg_ref_ext.py) under the project's accuracy rule: the device lies within
100 max(err_ref, 1e-15) of the extended result on the scale max(1, max |quantity|), err_ref the fp64 restatement's own
distance from it on the same inputs; determinants and weights relative.  Every comparison prints its three figures
(err_ref, device error, bound).  Shapes: M = 7 (under one MFMA tile), 19 (one tile + 3), 27, 33 (two tiles + 1)."""
import os

import numpy
import pytest

from pauxy_amd import _lib as L
from tests import thermal_ueg_ref as ur
from tests import thermal_ueg_ref_ext as ue
from tests.thermal_ueg_cases import ECUT_OF_M, Case

pytestmark = pytest.mark.gpu


def check(label, got, want64, want_ext, relative=False, factor=1.0):
    """device within factor x bound(err_ref) of the extended result."""
    if relative:
        err_ref, err_dev = ue.rerr(want64, want_ext), ue.rerr(got, want_ext)
    else:
        scale = max(1.0, float(numpy.max(numpy.abs(ue.ext(want_ext)))))
        err_ref, err_dev = ue.gerr(want64, want_ext, scale), ue.gerr(got, want_ext, scale)
    bnd = factor * ue.bound(err_ref)
    print("%s: err_ref %.3e device %.3e bound %.3e fraction %.3f" % (label, err_ref, err_dev, bnd, err_dev / bnd))
    _MEASURED.append((_GROUP[0], label, err_ref, err_dev, bnd))
    assert numpy.all(numpy.isfinite(numpy.asarray(got, dtype=complex))), label
    assert err_dev <= bnd, (label, err_ref, err_dev, bnd)


_MEASURED, _GROUP = [], [""]


@pytest.fixture(autouse=True)
def _group(request):
    _GROUP[0] = request.node.name
    yield


@pytest.fixture(scope="module", autouse=True)
def precision_table():
    """With THERMAL_UEG_PRECISION_OUT=<file> the module writes what it measured, the fraction of the bound per case, as
    the table kept in profiles/thermal_ueg_precision.md."""
    yield
    out = os.environ.get("THERMAL_UEG_PRECISION_OUT")
    if not out or not _MEASURED:
        return
    lines = ["# Thermal UEG walkers: measured fraction of the accuracy bound", "",
             "Written by `THERMAL_UEG_PRECISION_OUT=<this file> pytest tests/test_gpu_thermal_ueg.py` on an MI355X.  The rule",
             "(tests/itcf_ref_ext.py): the device lies within bound = 100 x max(err_ref, 1e-15) of the `numpy.clongdouble`",
             "restatement, err_ref the fp64 restatement's own distance from it on the same inputs, on the scale",
             "max(1, max |quantity|); determinants, M0 and weights relative.  fraction = device error / bound.  The rule was",
             "not tightened after these measurements.  Tests that compare after every slice are given by their worst slice",
             "per quantity.", "",
             "| test | comparison | err_ref | device | bound | fraction |", "|---|---|---|---|---|---|"]
    worst = {}
    for group, label, err_ref, err_dev, bnd in _MEASURED:
        words = label.split()
        key = (group, words[2] if words[0] == "slice" else label)
        if key not in worst or err_dev / bnd > worst[key][2] / worst[key][3]:
            worst[key] = (label, err_ref, err_dev, bnd)
    for (group, _), (label, err_ref, err_dev, bnd) in worst.items():
        lines.append("| %s | %s | %.2e | %.2e | %.2e | %.3f |" % (group, label, err_ref, err_dev, bnd, err_dev / bnd))
    lines += ["", "Largest fraction over every comparison of the module: %.3f." % max(e / b for _, _, _, e, b in _MEASURED), ""]
    with open(out, "w") as f:
        f.write("\n".join(lines))


_CASES = {}


def case_of(M):
    """One Case per basis size for the whole module (the operators are built once)."""
    if M not in _CASES:
        _CASES[M] = Case(ECUT_OF_M[M], 2 if M > 7 else 1)
    return _CASES[M]


# ---- the Green's function and its determinant alone, on uploaded bins
def greens_case(M, nbins, stack_size, slice_ixs, nw, seed=5, spread=20.0):
    c = case_of(M)
    stack = c.random_stack(nw, nbins, stack_size, seed, spread)
    dev = c.device(nw, stack_size, L=nbins * stack_size)
    try:
        dev.set(L.F_THERMAL_STACK, stack)
        numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_STACK), stack)
        for slice_ix in slice_ixs:
            dev.thermal_greens(slice_ix)
            G, det = dev.get(L.F_THERMAL_G), dev.get(L.F_THERMAL_DET)
            order = ur.chain_order(slice_ix, stack_size, nbins)
            bins = [stack[:, b].reshape(nw * 2, M, M) for b in order]
            G64 = ur.strat_greens(bins).reshape(G.shape)
            Gx = ue.strat_greens(bins).reshape(G.shape)
            tag = "M=%d nbins=%d ss=%d nw=%d slice_ix=%d" % (M, nbins, stack_size, nw, slice_ix)
            check("G " + tag, G, G64, Gx)
            check("det " + tag, det, ur.Kit64.det(G64), ue.det(Gx), relative=True)
    finally:
        dev.close()


@pytest.mark.parametrize("nbins", [1, 2, 5, 10])
@pytest.mark.parametrize("M", [7, 19, 27, 33])
def test_stratified_greens_and_determinant_from_uploaded_bins(M, nbins):
    greens_case(M, nbins, 5, [0], nw=3 if M < 33 else 1)


@pytest.mark.parametrize("M,nbins,stack_size", [(7, 5, 2), (19, 1, 10), (19, 2, 5), (19, 10, 1), (33, 5, 2)])
def test_stratified_greens_every_starting_slice(M, nbins, stack_size):
    """Every slice_ix of 1, 2, 5 and 10 bins, under and over one MFMA tile; the final one (bin_ix == nbins -> the chain
    starts at bin 0) included."""
    greens_case(M, nbins, stack_size, list(range(0, nbins * stack_size + 1)), nw=1)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_stratified_greens_of_the_fixtures_bins(golden, k):
    """The bins of the reference's walkers (cases a1, a2, a3: M = 7 / 19 / 33 with 10 / 2 / 5 bins) after every slice,
    rebuilt from the recorded fields by the fp64 restatement and uploaded through afq_walkers_set: G and det of the
    Green's kernel alone under the rule, and G against the reference's own record."""
    d = golden("thermal_ueg.npz")
    c, pre = a_case(d, k)
    ss, M = int(d[pre + 'stack_size']), c.M
    p = c.path64(ss, 1)
    stacks = []
    for ts in range(c.L):
        p.step(d[pre + 'xi'][ts][None])
        stacks.append(p.stack[0].copy())
    stacks = numpy.array(stacks)                                  # one "walker" per slice of the path
    nbins = c.L // ss
    dev = c.device(c.L, ss)
    try:
        dev.set(L.F_THERMAL_STACK, stacks)
        dev.thermal_greens(c.L)
        G, det = dev.get(L.F_THERMAL_G), dev.get(L.F_THERMAL_DET)
        bins = [stacks[:, b].reshape(c.L * 2, M, M) for b in ur.chain_order(c.L, ss, nbins)]
        G64, Gx = ur.strat_greens(bins).reshape(G.shape), ue.strat_greens(bins).reshape(G.shape)
        check("G of the bins of a%d" % k, G, G64, Gx)
        check("det of the bins of a%d" % k, det, ur.Kit64.det(G64), ue.det(Gx), relative=True)
        assert ue.gerr(G, d[pre + 'G']) <= 1e-10
        assert ue.rerr(det, d[pre + 'M0']) <= 1e-10
    finally:
        dev.close()


@pytest.mark.parametrize("M", [19, 33])
def test_stratified_greens_hardest_bins(M):
    """4 bins of 20 slices whose one-body exponents spread over 20 / dt: bins of condition 1e8."""
    c = case_of(M)
    stack = c.random_stack(1, 1, 20, 5)
    assert numpy.linalg.cond(stack[0, 0, 0]) > 1e7
    greens_case(M, 4, 20, [0, 40], nw=1)


def test_stratified_greens_of_65_walkers():
    greens_case(7, 2, 5, [0], nw=65)


# ---- one slice after another against case (a) of the fixture
def a_case(d, k):
    pre = 'a%d_' % k
    c = Case(float(d[pre + 'ecut']), int(d[pre + 'nelec']), rs=float(d[pre + 'rs']), beta=float(d[pre + 'beta']),
             dt=float(d[pre + 'dt']), mu=float(d[pre + 'mu_system']), fb_bound=float(d[pre + 'fb_bound']))
    return c, pre


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_single_walker_slice_by_slice(golden, k):
    """The recorded fields of the reference's walker through afq_thermal_propagate_continuous, beside a second walker
    with fields of its own: xbar, cmf, cfb at 1e-12; right, the bins, G, M0 and the weight under the rule after every
    slice; the reference's own record; the final energies and nav.  k = 4: the force-bias clip fires."""
    d = golden("thermal_ueg.npz")
    c, pre = a_case(d, k)
    ss, M = int(d[pre + 'stack_size']), c.M
    rng = numpy.random.RandomState(40 + k)
    p64, px = c.path64(ss, 2), c.path_ext(ss, 2)
    dev = c.device(2, ss)
    try:
        check("trial G", dev.get(L.F_THERMAL_G), p64.G, px.G)
        check("trial M0", dev.get(L.F_THERMAL_M0), p64.M0, px.M0, relative=True)
        for ts in range(c.L):
            xi = numpy.array([d[pre + 'xi'][ts], rng.normal(size=c.K)])
            xb64, cmf64, cfb64 = p64.step(xi)
            xbx, cmfx, cfbx = px.step(xi)
            used = dev.thermal_propagate_continuous(xi, fetch_fields=True)
            numpy.testing.assert_array_equal(used, xi)
            assert dev.thermal_state() == (px.time_slice, px.block, px.counter, px.nbins)
            tag = "slice %d " % (ts + 1)
            for name, got, want in (("xbar", dev.get(L.F_XBAR), xbx), ("cmf", dev.get(L.F_CMF), cmfx),
                                    ("cfb", dev.get(L.F_CFB), cfbx)):
                err = ue.gerr(got, want)
                print("%s%s: %.3e (tolerance 1e-12)" % (tag, name, err))
                assert err <= 1e-12, (tag, name, err)
            assert ue.gerr(dev.get(L.F_XBAR)[0], d[pre + 'xbar'][ts]) <= 1e-12
            check(tag + "right", dev.get(L.F_THERMAL_RIGHT), p64.right, px.right)
            check(tag + "bins", dev.get(L.F_THERMAL_STACK), p64.stack, px.stack)
            G = dev.get(L.F_THERMAL_G)
            check(tag + "G", G, p64.G, px.G)
            check(tag + "M0", dev.get(L.F_THERMAL_M0), p64.M0, px.M0, relative=True)
            w = dev.get(L.F_WEIGHT)
            check(tag + "weight", w, p64.weight, px.weight, relative=True)
            assert abs(w[0] / d[pre + 'weight'][ts] - 1) <= 1e-10              # and the reference's own record
            assert ue.gerr(G[0], d[pre + 'G'][ts]) <= 1e-10
        assert px.min_cos_margin > 1e-6
        assert (int(dev.counters()[0]) > 0) == (k == 4) and p64.nclip == px.nclip
        if k == 4:
            assert int(dev.counters()[0]) == px.nclip
        E, nav = dev.thermal_energy()
        E64, nav64 = p64.energy()
        Ex, navx = px.energy()
        scale = float(numpy.max(numpy.abs(c.ops.H1diag))) * M + float(numpy.sum(c.ops.vqvec)) / c.system.vol * M
        check("energy", E, E64.real, Ex.real, factor=scale)
        check("nav", nav, nav64.real, navx.real, factor=M)
        assert ue.gerr(E[0], d[pre + 'energy'].real) <= 1e-10
        assert abs(nav[0] - complex(d[pre + 'nav']).real) <= 1e-10
        with pytest.raises(L.AfqError) as e:                                   # the path is complete
            dev.thermal_propagate_continuous(xi)
        assert e.value.code == L.AFQ_ESTATE
    finally:
        dev.close()


def test_kill_branches_of_the_weight_update(golden):
    """Walker 1: M0 huge, so that the determinant ratio overflows (magn = inf): weight 0 and M0 kept.  Walker 2: the
    sign of one M0 flipped, so that the ratio is negative (cos = -1): weight 0 and M0 updated.  Walker 3: M0 not a
    number: weight 0 (not NaN, which the comb's total would inherit) and M0 kept.  Walker 0 untouched."""
    c = case_of(7)
    dev = c.device(4, 5)
    try:
        xi = numpy.random.RandomState(3).normal(size=(4, c.K))
        M0 = dev.get(L.F_THERMAL_M0)
        huge = numpy.array([1e200 + 0j, 1e200 + 0j])
        M0[1] = huge
        M0[2, 0] = -M0[2, 0]
        M0[3, 1] = numpy.nan
        dev.set(L.F_THERMAL_M0, M0)
        dev.thermal_propagate_continuous(xi)
        w, M1, det = dev.get(L.F_WEIGHT), dev.get(L.F_THERMAL_M0), dev.get(L.F_THERMAL_DET)
        assert w[0] > 0 and w[1] == 0.0 and w[2] == 0.0 and w[3] == 0.0
        numpy.testing.assert_array_equal(M1[1], huge)
        assert numpy.isnan(M1[3, 1]) and M1[3, 0] == M0[3, 0]
        numpy.testing.assert_array_equal(M1[0], det[0])
        numpy.testing.assert_array_equal(M1[2], det[2])
        assert numpy.all(numpy.abs(det) > 0)
    finally:
        dev.close()


# ---- whole paths through the Python classes, numpy.random replayed
def b_options(d, k):
    pre = 'b%d_' % k
    return pre, {'qmc': {'timestep': float(d[pre + 'dt']), 'beta': float(d[pre + 'beta']),
                         'num_walkers': int(d[pre + 'nwalkers']), 'blocks': 2,
                         'pop_control_freq': int(d[pre + 'npop_control']), 'rng_seed': int(d[pre + 'seed'])},
                 'model': {'name': 'UEG', 'rs': 1.0, 'ecut': float(d[pre + 'ecut']), 'nup': int(d[pre + 'nelec']),
                           'ndown': int(d[pre + 'nelec']), 'mu': float(d[pre + 'mu_system'])},
                 'trial': {'name': 'one_body'},
                 'walkers': {'stack_size': int(d[pre + 'stack_size']), 'low_rank': False},
                 'estimates': {'mixed': {'verbose': False}}}


def run_driver(options, record_state=False):
    """-> (rows, weights after every slice before its cap, parents of every comb, walker state after every comb)."""
    from pauxy_amd.context import release_context
    from pauxy_amd.qmc.thermal_afqmc import ThermalAFQMC
    state = numpy.random.get_state()
    afqmc = ThermalAFQMC(options=options)
    try:
        walk, prop = afqmc.walk, afqmc.propagators
        weights, parents, states = [], [], []
        move, comb = prop.propagate_walkers, walk.pop_control

        def propagate_walkers(w, eshift=0):
            move(w, eshift)
            weights.append(walk.dev.get(L.F_WEIGHT))

        def pop_control(comm=None):
            before = [walk.dev.get(f) for f in (L.F_THERMAL_G, L.F_THERMAL_STACK, L.F_THERMAL_RIGHT, L.F_THERMAL_M0)]
            comb(comm)
            parents.append(numpy.array(walk.last_parent_ix))
            if record_state:
                after = [walk.dev.get(f) for f in (L.F_THERMAL_G, L.F_THERMAL_STACK, L.F_THERMAL_RIGHT, L.F_THERMAL_M0)]
                states.append((before, after))
        prop.propagate_walkers, walk.pop_control = propagate_walkers, pop_control
        afqmc.run()
        mixed = afqmc.estimators.estimators['mixed']
        return (numpy.array(mixed.blocks).real, list(mixed.header), numpy.array(weights), parents, states,
                numpy.random.random())
    finally:
        numpy.random.set_state(state)
        release_context(afqmc.system, afqmc.trial)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_golden_driver_paths(golden, k):
    """Case (b): ThermalAFQMC over two paths from the seed of the reference's run: its comb parents exactly, its
    estimator rows to 1e-9, its weights after every slice; the weights after every slice and the rows under the rule
    against the extended restatement of the same run (stored: thermal_ueg_paths_ext.npz); a clone carries G, the bins,
    right and M0 of its parent bit for bit; the stream is consumed exactly as the reference consumed it."""
    d = golden("thermal_ueg.npz")
    x = golden("thermal_ueg_paths_ext.npz")
    pre, options = b_options(d, k)
    rows, header, weights, parents, states, nxt = run_driver(options, record_state=True)
    numpy.testing.assert_array_equal(numpy.array(parents), x[pre + 'parents'])
    check("weights b%d" % k, weights, x[pre + 'w64'], ue.LD(1) * x[pre + 'wx_hi'] + x[pre + 'wx_lo'], relative=True)
    check("rows b%d" % k, rows[:, 1:11], x[pre + 'r64'], ue.LD(1) * x[pre + 'rx_hi'] + x[pre + 'rx_lo'])
    assert header == list(d[pre + 'header'])
    numpy.testing.assert_array_equal(numpy.array(parents), d[pre + 'parent_ix'])
    gold = d[pre + 'blocks'].real
    assert rows.shape == gold.shape == (3, 12)
    scale = max(1.0, float(numpy.max(numpy.abs(gold[:, 1:11]))))
    err = float(numpy.max(numpy.abs(rows[:, :11] - gold[:, :11]))) / scale
    print("rows: %.3e (tolerance 1e-9)" % err)
    assert err <= 1e-9
    werr = float(numpy.max(numpy.abs(weights / d[pre + 'weights'] - 1)))
    print("weights: %.3e (tolerance 1e-10)" % werr)
    assert werr <= 1e-10
    nclone = 0
    for parent, (before, after) in zip(parents, states):
        want = [b.copy() for b in before]
        for cl, kl in zip(numpy.where(parent > 1)[0], numpy.where(parent == 0)[0]):
            for x, b in zip(want, before):
                x[kl] = b[cl]
            nclone += 1
        for x, a in zip(want, after):
            numpy.testing.assert_array_equal(x, a)
    assert nclone > 0
    # the next uniform is the next of the seed's stream
    rs = numpy.random.RandomState(int(d[pre + 'seed']))
    nw, K, Lts = int(d[pre + 'nwalkers']), weights.shape[0], int(d[pre + 'ntime_slices'])
    nfields = 2 * len(case_of(19 if k < 2 else 33).system.qvecs)
    for _ in range(2):
        for ts in range(Lts):
            rs.normal(0.0, 1.0, (nw, nfields))
            if ts % int(d[pre + 'npop_control']) == 0 and ts != 0:
                rs.random_sample()
    assert K == 2 * Lts and nxt == rs.random_sample()


def test_driver_path_repeated_gives_the_same_bits(golden):
    d = golden("thermal_ueg.npz")
    pre, options = b_options(d, 1)
    rows, _, weights, parents, _, _ = run_driver(options)
    rows2, _, weights2, parents2, _, _ = run_driver(options)
    numpy.testing.assert_array_equal(rows[:, :11], rows2[:, :11])
    numpy.testing.assert_array_equal(weights, weights2)
    numpy.testing.assert_array_equal(numpy.array(parents), numpy.array(parents2))


def test_reset_path_reset_reproduces_the_path_bit_for_bit():
    c = case_of(19)
    nw = 5
    xis = numpy.random.RandomState(9).normal(size=(c.L, nw, c.K))
    dev = c.device(nw, 5)
    try:
        M00 = dev.get(L.F_THERMAL_M0)
        runs = []
        for _ in range(2):
            dev.thermal_reset()
            dev.set(L.F_THERMAL_M0, M00)              # (a reset leaves M0 where the last path ended, as the reference does)
            assert dev.thermal_state() == (0, 0, 0, 2)
            numpy.testing.assert_array_equal(dev.get(L.F_WEIGHT), numpy.ones(nw))
            out = []
            for ts in range(c.L):
                dev.thermal_propagate_continuous(xis[ts])
                out.append([dev.get(f) for f in (L.F_THERMAL_G, L.F_THERMAL_STACK, L.F_THERMAL_RIGHT, L.F_THERMAL_M0,
                                                 L.F_WEIGHT)])
            runs.append(out)
        for a, b in zip(*runs):
            for x, y in zip(a, b):
                numpy.testing.assert_array_equal(x, y)
        M1 = dev.get(L.F_THERMAL_M0)
        dev.thermal_reset()
        numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_M0), M1)
    finally:
        dev.close()


def test_device_philox_fields():
    """xi = NULL: two runs with the same seed are bitwise equal, and the fields read back and fed as xi reproduce the
    run."""
    c = case_of(19)
    nw = 4
    dev = c.device(nw, 5)
    try:
        runs = []
        M00 = dev.get(L.F_THERMAL_M0)
        for mode in ("draw", "draw", "feed"):
            dev.rng_seed(1234, 0)
            dev.thermal_reset()
            dev.set(L.F_THERMAL_M0, M00)
            out, fields = [], []
            for ts in range(4):
                xi = None if mode == "draw" else runs[0][1][ts]
                fields.append(dev.thermal_propagate_continuous(xi, fetch_fields=True))
                out.append([dev.get(f) for f in (L.F_THERMAL_G, L.F_THERMAL_STACK, L.F_THERMAL_M0, L.F_WEIGHT)])
            runs.append((out, fields))
        f = numpy.array(runs[0][1])
        assert abs(f.mean()) < 0.05 and abs(f.std() - 1) < 0.05 and len(numpy.unique(f)) == f.size
        for other in runs[1:]:
            numpy.testing.assert_array_equal(numpy.array(other[1]), f)
            for a, b in zip(runs[0][0], other[0]):
                for x, y in zip(a, b):
                    numpy.testing.assert_array_equal(x, y)
    finally:
        dev.close()


# ---- neighbours: the Hubbard thermal handle and a ground-state UEG handle are what they were
def hubbard_thermal_result():
    from tests.thermal_cases import Case as HCase
    case = HCase(3, 2, 4.0, 0.05, mu=1.0, mu_trial=0.8)
    rng = numpy.random.RandomState(17)
    dev = case.device(5, 10, 5, 5)
    try:
        out = []
        for ts in range(10):
            out.append(dev.thermal_propagate(rng.random_sample((5, case.M)), 0.0, fetch_fields=True))
        out += [dev.get(L.F_THERMAL_G), dev.get(L.F_THERMAL_STACK), dev.get(L.F_WEIGHT)]
        out += list(dev.thermal_energy())
        dev.set(L.F_WEIGHT, numpy.array([0.05, 2.6, 1.0, 0.1, 1.2]))
        out += [dev.popcontrol_comb(0.37, 5)[0], dev.get(L.F_THERMAL_G), dev.get(L.F_THERMAL_STACK)]
        return out
    finally:
        dev.close()


def ueg_ground_state_result(golden):
    from tests.helpers import make_device, ueg_model
    d = golden('ueg_ops.npz')
    m = ueg_model(d, 'U_')
    dev = make_device(m, 2)
    try:
        dev.set(L.F_PHI, numpy.array([d['pw_phi'], d['pw_phi']]))
        dev.greens(want_G=True)
        xi = numpy.random.RandomState(2).normal(size=(2, dev.K))
        dev.propagate(xi, 0.0)
        return [dev.get(L.F_PHI), dev.get(L.F_WEIGHT), dev.get(L.F_XBAR), dev.local_energy()]
    finally:
        dev.close()


def test_neighbours_are_unchanged_by_a_thermal_ueg_handle(golden):
    before = hubbard_thermal_result() + ueg_ground_state_result(golden)
    c = case_of(19)
    dev = c.device(3, 5)
    try:
        dev.thermal_propagate_continuous(numpy.random.RandomState(1).normal(size=(3, c.K)))
        mid = hubbard_thermal_result() + ueg_ground_state_result(golden)       # with the handle alive
    finally:
        dev.close()
    after = hubbard_thermal_result() + ueg_ground_state_result(golden)
    for other in (mid, after):
        assert len(other) == len(before)
        for x, y in zip(before, other):
            numpy.testing.assert_array_equal(x, y)


# ---- refusals on the device, each by code and name
def refused(fn, code=None):
    with pytest.raises(L.AfqError) as e:
        fn()
    assert e.value.code == (L.AFQ_EUNSUPPORTED if code is None else code), e.value
    return str(e.value)


def test_m_57_is_refused_with_the_number():
    text = refused(lambda: Case(2.5, 2).device(1, 5))
    assert "57" in text and "47" in text


@pytest.mark.parametrize("bit,word", [(L.THERMAL_FREE_PROJECTION, "free_projection"), (L.THERMAL_LOW_RANK, "low_rank"),
                                      (L.THERMAL_AVERAGE_GF, "average_gf")])
def test_option_is_refused(bit, word):
    assert word in refused(lambda: case_of(7).device(1, 5, options=bit))


def test_windows_rdm_pair_branch_and_the_other_propagate_are_refused():
    dev = case_of(7).device(4, 5)
    try:
        assert "back-propagation" in refused(lambda: dev.bp_configure(4))
        assert "ITCF" in refused(lambda: dev.itcf_configure(2))
        assert "rdm" in refused(lambda: dev.estimates_rdm(True))
        assert "pair_branch" in refused(lambda: dev.popcontrol_pair_branch(numpy.full(2, 0.5), 4, 0.1, 4.0))
        assert "continuous" in refused(lambda: dev.thermal_propagate(numpy.full((4, 7), 0.5)), L.AFQ_ESTATE)
        for field in (L.F_THERMAL_DET, L.F_CMF, L.F_CFB):             # results of the last kernel: get only
            assert "get only" in refused(lambda: dev.set(field, dev.get(field)), L.AFQ_EINVAL)
    finally:
        dev.close()


def test_two_ranks_are_refused():
    from pauxy_amd import device as devmod
    c = case_of(7)
    s = c.system
    ranks = [devmod.AfqDevice(0) for _ in range(2)]
    try:
        for dev in ranks:
            dev.set_system_ueg(s.iA, s.iB, s.ikpq_i, s.ikpq_kpq, s.ipmq_i, s.ipmq_pmq, s.vqvec, s.vol,
                               numpy.array([s.H1[0].diagonal(), s.H1[1].diagonal()]), s.ecore, s.nup, s.ndown)
            dev.walkers_alloc(2)
        devmod.comm_init_local(ranks)
        assert "one rank" in refused(lambda: ranks[0].thermal_configure_continuous(
            c.L, 5, c.dt, c.full(c.BT), c.full(c.BT_inv), c.full(c.BH1), c.mf_shift))
    finally:
        for dev in ranks:
            dev.close()


def test_other_systems_a_dense_trial_and_a_bad_stack_size_are_refused():
    from tests.thermal_cases import Case as HCase
    c = case_of(7)
    h = HCase(2, 2, 4.0, 0.05)
    from pauxy_amd.device import AfqDevice
    dev = AfqDevice(0)
    try:
        dev.set_system_hubbard(h.H1.astype(complex), h.U, h.na, h.nb)
        dev.walkers_alloc(2)
        eye = numpy.array([numpy.eye(4)] * 2)
        assert "UEG" in refused(lambda: dev.thermal_configure_continuous(10, 5, 0.05, eye, eye, eye, numpy.zeros(dev.K)))
    finally:
        dev.close()
    dense = c.full(c.BT) + 1e-3
    assert "diagonal" in refused(lambda: c.device(1, 5, BT=dense))
    refused(lambda: c.device(1, 3), L.AFQ_EINVAL)                 # stack_size does not divide the slices
    # a Hubbard handle is still refused by afq_thermal_configure's words when it is not Hubbard
    s = c.system
    dev = AfqDevice(0)
    try:
        dev.set_system_ueg(s.iA, s.iB, s.ikpq_i, s.ikpq_kpq, s.ipmq_i, s.ipmq_pmq, s.vqvec, s.vol,
                           numpy.array([s.H1[0].diagonal(), s.H1[1].diagonal()]), s.ecore, s.nup, s.ndown)
        dev.walkers_alloc(2)
        eye = numpy.array([numpy.eye(c.M)] * 2)
        assert "Hubbard" in refused(lambda: dev.thermal_configure(10, 5, 5, eye, eye, eye, numpy.ones((2, 2))))
        refused(lambda: dev.thermal_propagate_continuous(None), L.AFQ_ESTATE)      # not configured
    finally:
        dev.close()
