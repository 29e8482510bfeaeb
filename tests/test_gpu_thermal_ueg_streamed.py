"""The streamed Green's function of the thermal UEG walkers (AFQ_THERMAL_STREAMED_GREENS: W and Qt in LDS, T in device
memory), which carries the path to the M = 57 shell, under the rule of tests/test_gpu_thermal_ueg.py: the device lies
within 100 max(err_ref, 1e-15) of the numpy.clongdouble restatement (tests/thermal_ueg_ref_ext.py) on the scale
max(1, max |quantity|), err_ref the fp64 restatement's own distance from it on the same inputs; determinants, M0 and
weights relative.  Every comparison prints err_ref, device error and bound.  Every handle here is made with
options=L.THERMAL_STREAMED_GREENS unless the test sets the two engines side by side.  Shapes: M = 7 (under one MFMA tile),
19 (tile + 3), 33 (two tiles + 1), 57 (three tiles + 9, the 117 KB layout).

With THERMAL_UEG_STREAMED_PRECISION_OUT=<file> the module writes what it measured
(profiles/thermal_ueg_streamed_precision.md)."""
import os

import numpy
import pytest

from pauxy_amd import _lib as L
from tests import thermal_ueg_ref as ur
from tests import thermal_ueg_ref_ext as ue
from tests.thermal_ueg_cases import ECUT_OF_M, Case

pytestmark = pytest.mark.gpu

BIT = getattr(L, "THERMAL_STREAMED_GREENS", 16)          # (a library without the option refuses the bit: every test fails)
STREAMED, RESIDENT = "thermal_cgreens_streamed_kernel", "thermal_cgreens_kernel"
WALKER_FIELDS = (L.F_THERMAL_G, L.F_THERMAL_STACK, L.F_THERMAL_RIGHT, L.F_THERMAL_M0, L.F_WEIGHT)

_MEASURED, _GROUP, _ENGINES = [], [""], []


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


@pytest.fixture(autouse=True)
def _group(request):
    _GROUP[0] = request.node.name
    yield


@pytest.fixture(scope="module", autouse=True)
def precision_table():
    yield
    out = os.environ.get("THERMAL_UEG_STREAMED_PRECISION_OUT")
    if not out or not _MEASURED:
        return
    lines = ["# Thermal UEG walkers, streamed Green's function: measured fraction of the accuracy bound", "",
             "Written by `THERMAL_UEG_STREAMED_PRECISION_OUT=<this file> pytest tests/test_gpu_thermal_ueg_streamed.py` on an",
             "MI355X.  The rule (tests/itcf_ref_ext.py): the device lies within bound = 100 x max(err_ref, 1e-15) of the",
             "`numpy.clongdouble` restatement, err_ref the fp64 restatement's own distance from it on the same inputs, on the",
             "scale max(1, max |quantity|); determinants, M0 and weights relative.  fraction = device error / bound.  The",
             "rule was not tightened after these measurements.  Tests that compare after every slice, at every starting",
             "slice or walker by walker are given by their worst comparison per quantity.", "",
             "| test | comparison | err_ref | device | bound | fraction |", "|---|---|---|---|---|---|"]
    worst = {}
    for group, label, err_ref, err_dev, bnd in _MEASURED:
        words = label.split()
        key = (group, words[2] if words[0] == "slice" else words[0] if words[0] in ("G", "det") else label)
        if key not in worst or err_dev / bnd > worst[key][2] / worst[key][3]:
            worst[key] = (label, err_ref, err_dev, bnd)
    for (group, _), (label, err_ref, err_dev, bnd) in worst.items():
        lines.append("| %s | %s | %.2e | %.2e | %.2e | %.3f |" % (group, label, err_ref, err_dev, bnd, err_dev / bnd))
    lines += ["", "Largest fraction over every comparison of the module: %.3f." % max(e / b for _, _, _, e, b in _MEASURED), ""]
    if _ENGINES:
        lines += ["The streamed and the resident engine, side by side on the same inputs (largest |difference| per quantity;",
                  "the tests assert equal bits):", "", "| test | quantity | largest difference |", "|---|---|---|"]
        largest = {}
        for group, quantity, diff in _ENGINES:
            key = (group, quantity.split()[0])
            largest[key] = max(largest.get(key, 0.0), diff)
        lines += ["| %s | %s | %.2e |" % (group, quantity, diff) for (group, quantity), diff in largest.items()]
        lines.append("")
    with open(out, "w") as f:
        f.write("\n".join(lines))


_CASES = {}


def case_of(M):
    """One Case per basis size for the whole module (the operators are built once)."""
    if M not in _CASES:
        _CASES[M] = Case(ECUT_OF_M[M], 2 if M > 7 else 1)
    return _CASES[M]


def launched(dev):
    """Names of the Green's kernels in the handle's launch trace."""
    return set(n for n in dev.launch_trace_get() if n in (STREAMED, RESIDENT))


# ---- 1 .. 4: the Green's function and its determinant alone, on uploaded bins
def greens_case(M, nbins, stack_size, slice_ixs, nw, seed=5, spread=20.0, twice=False):
    c = case_of(M)
    stack = c.random_stack(nw, nbins, stack_size, seed, spread)
    dev = c.device(nw, stack_size, options=BIT, L=nbins * stack_size)
    try:
        dev.set(L.F_THERMAL_STACK, stack)
        numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_STACK), stack)
        refs = {}                                               # slices of one bin share their chain
        for slice_ix in slice_ixs:
            dev.thermal_greens(slice_ix)
            G, det = dev.get(L.F_THERMAL_G), dev.get(L.F_THERMAL_DET)
            order = tuple(ur.chain_order(slice_ix, stack_size, nbins))
            if order not in refs:
                bins = [stack[:, b].reshape(nw * 2, M, M) for b in order]
                refs[order] = (ur.strat_greens(bins).reshape(G.shape), ue.strat_greens(bins).reshape(G.shape))
            G64, Gx = refs[order]
            tag = "M=%d nbins=%d ss=%d nw=%d slice_ix=%d" % (M, nbins, stack_size, nw, slice_ix)
            if nw > 3:                                          # every walker under the rule by itself
                for w in range(nw):
                    check("G walker %d %s" % (w, tag), G[w], G64[w], Gx[w])
                    check("det walker %d %s" % (w, tag), det[w], ur.Kit64.det(G64[w]), ue.det(Gx[w]), relative=True)
            else:
                check("G " + tag, G, G64, Gx)
                check("det " + tag, det, ur.Kit64.det(G64), ue.det(Gx), relative=True)
            if twice:
                dev.thermal_greens(slice_ix)
                numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_G), G)
                numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_DET), det)
    finally:
        dev.close()


@pytest.mark.parametrize("nbins", [1, 2, 5, 10])
@pytest.mark.parametrize("M", [7, 19, 33, 57])
def test_streamed_greens_and_determinant_from_uploaded_bins(M, nbins):
    """nbins = 1: no chain product, T goes from the first QR straight to the closing step.  Three distinct walkers."""
    greens_case(M, nbins, 5, [0], nw=3)


@pytest.mark.parametrize("nbins,stack_size", [(2, 5), (5, 2)])
def test_streamed_greens_every_starting_slice_at_57(nbins, stack_size):
    """Every slice_ix from 0 to L: the rotation of `first`, and the final one (bin_ix == nbins -> the chain starts at
    bin 0)."""
    greens_case(57, nbins, stack_size, list(range(0, nbins * stack_size + 1)), nw=1)


def test_streamed_greens_hardest_bins_at_57():
    """4 bins of 20 slices whose one-body exponents spread over 20 / dt."""
    c = case_of(57)
    stack = c.random_stack(1, 1, 20, 5)
    cond = numpy.linalg.cond(stack[0, 0, 0])
    print("condition of a bin: %.3e" % cond)
    assert cond > 1e7
    greens_case(57, 4, 20, [0, 80], nw=1)


@pytest.mark.parametrize("M,nw", [(19, 33), (57, 9)])
def test_scratch_is_per_work_group(M, nw):
    """Distinct walkers in one launch, each under the rule: work-groups that share or overrun a scratch buffer fail
    here.  The same call twice gives the same bits."""
    greens_case(M, 2, 5, [0], nw=nw, twice=True)


# ---- 5: the two engines
def note_engines(quantity, a, b):
    a, b = numpy.asarray(a), numpy.asarray(b)
    _ENGINES.append((_GROUP[0], quantity, float(numpy.max(numpy.abs(a - b))) if a.size else 0.0))


@pytest.mark.parametrize("nbins", [1, 2, 5])
@pytest.mark.parametrize("M", [7, 19, 33])
def test_the_two_engines_agree_on_uploaded_bins(M, nbins):
    c = case_of(M)
    stack = c.random_stack(3, nbins, 5, 5)
    out = []
    for options, mine, other in ((BIT, STREAMED, RESIDENT), (0, RESIDENT, STREAMED)):
        dev = c.device(3, 5, options=options, L=nbins * 5)
        try:
            dev.launch_trace(True)
            dev.set(L.F_THERMAL_STACK, stack)
            dev.thermal_greens(0)
            out.append((dev.get(L.F_THERMAL_G), dev.get(L.F_THERMAL_DET)))
            assert launched(dev) == {mine}, (launched(dev), other)
        finally:
            dev.close()
    for name, a, b in zip(("G", "det"), out[0], out[1]):
        note_engines("%s M=%d nbins=%d" % (name, M, nbins), a, b)
    numpy.testing.assert_array_equal(out[0][0], out[1][0])
    numpy.testing.assert_array_equal(out[0][1], out[1][1])


def test_the_two_engines_agree_over_a_path():
    """A whole 10-slice path of 3 walkers at M = 19: G, bins, right, M0 and weights after every slice, bit for bit; the
    launch trace holds the streamed kernel's name for the handle with the bit and never the resident one's, and the
    reverse for the default handle (a reset, the slices and afq_thermal_greens)."""
    c = case_of(19)
    xis = numpy.random.RandomState(21).normal(size=(c.L, 3, c.K))
    runs = []
    for options, mine in ((BIT, STREAMED), (0, RESIDENT)):
        dev = c.device(3, 5, options=options)
        try:
            dev.launch_trace(True)
            dev.thermal_reset()
            out = [[dev.get(f) for f in WALKER_FIELDS]]
            for ts in range(c.L):
                dev.thermal_propagate_continuous(xis[ts])
                out.append([dev.get(f) for f in WALKER_FIELDS])
            dev.thermal_greens(3)
            out.append([dev.get(L.F_THERMAL_G), dev.get(L.F_THERMAL_DET)])
            assert launched(dev) == {mine}
            runs.append(out)
        finally:
            dev.close()
    for n, (a, b) in enumerate(zip(*runs)):
        names = ("G", "bins", "right", "M0", "weight") if len(a) == 5 else ("G(slice_ix=3)", "det(slice_ix=3)")
        for name, x, y in zip(names, a, b):
            note_engines("%s after slice %d" % (name, n), x, y)
    for a, b in zip(*runs):
        for x, y in zip(a, b):
            numpy.testing.assert_array_equal(x, y)


# ---- 6: one slice after another at M = 57 against case a5 of the fixture
def test_single_walker_slice_by_slice_at_57(golden):
    """The recorded fields of the reference's walker beside a second walker with fields of its own: xbar, cmf, cfb at
    1e-12; right, the bins, G, M0 and the weight under the rule after every slice; the reference's own weight after
    every slice and G after the odd ones (what the fixture holds) at 1e-10; the final energies and nav."""
    d = golden("thermal_ueg57.npz")
    pre = 'a5_'
    c = Case(float(d[pre + 'ecut']), int(d[pre + 'nelec']), rs=float(d[pre + 'rs']), beta=float(d[pre + 'beta']),
             dt=float(d[pre + 'dt']), mu=float(d[pre + 'mu_system']), fb_bound=float(d[pre + 'fb_bound']))
    ss, M = int(d[pre + 'stack_size']), c.M
    assert M == 57 and ss == 5
    stored = {int(n): i for i, n in enumerate(d[pre + 'G_slices'])}
    rng = numpy.random.RandomState(45)
    p64, px = c.path64(ss, 2), c.path_ext(ss, 2)
    dev = c.device(2, ss, options=BIT)
    try:
        check("trial G", dev.get(L.F_THERMAL_G), p64.G, px.G)
        check("trial M0", dev.get(L.F_THERMAL_M0), p64.M0, px.M0, relative=True)
        for ts in range(c.L):
            xi = numpy.array([d[pre + 'xi'][ts], rng.normal(size=c.K)])
            p64.step(xi)
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
            if ts + 1 in stored:
                assert ue.gerr(G[0], d[pre + 'G'][stored[ts + 1]]) <= 1e-10
        assert px.min_cos_margin > 1e-6
        assert int(dev.counters()[0]) == 0 and p64.nclip == px.nclip == 0
        E, nav = dev.thermal_energy()
        E64, nav64 = p64.energy()
        Ex, navx = px.energy()
        scale = float(numpy.max(numpy.abs(c.ops.H1diag))) * M + float(numpy.sum(c.ops.vqvec)) / c.system.vol * M
        check("energy", E, E64.real, Ex.real, factor=scale)
        check("nav", nav, nav64.real, navx.real, factor=M)
        assert ue.gerr(E[0], d[pre + 'energy'].real) <= 1e-10
        assert abs(nav[0] - complex(d[pre + 'nav']).real) <= 1e-10
    finally:
        dev.close()


# ---- 7: the driver at M = 57 against case b4 of the fixture
def test_golden_driver_paths_at_57(golden):
    """ThermalAFQMC with walkers: {stack_size: 5, streamed_greens: True} over two paths from the recorded seed: the
    reference's comb parents exactly, its estimator rows to 1e-9, its weights after every slice to 1e-10; a clone
    carries G, the bins, right and M0 of its parent bit for bit; the stream is consumed as the reference consumed it."""
    from tests.test_gpu_thermal_ueg import b_options, run_driver
    d = golden("thermal_ueg57.npz")
    pre, options = b_options(d, 4)
    options['walkers']['streamed_greens'] = True
    assert options['walkers']['stack_size'] == 5 and int(d[pre + 'seed']) >= 8
    rows, header, weights, parents, states, nxt = run_driver(options, record_state=True)
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
    rs = numpy.random.RandomState(int(d[pre + 'seed']))
    nw, Lts = int(d[pre + 'nwalkers']), int(d[pre + 'ntime_slices'])
    for _ in range(2):
        for ts in range(Lts):
            rs.normal(0.0, 1.0, (nw, case_of(57).K))
            if ts % int(d[pre + 'npop_control']) == 0 and ts != 0:
                rs.random_sample()
    assert weights.shape[0] == 2 * Lts and nxt == rs.random_sample()


# ---- 8: refusals and acceptances
def refused(fn, code=None):
    with pytest.raises(L.AfqError) as e:
        fn()
    assert e.value.code == (L.AFQ_EUNSUPPORTED if code is None else code), e.value
    return str(e.value)


def test_m_81_is_refused_with_the_bit_naming_the_slice_kernel():
    c = Case(3.0, 2)
    assert c.M == 81
    text = refused(lambda: c.device(1, 5, options=BIT))
    assert "81" in text and "57" in text and "slice kernel" in text and "thermal_cslice_kernel" in text


def test_hubbard_configure_refuses_the_bit_by_name():
    from tests.thermal_cases import Case as HCase
    assert "streamed_greens" in refused(lambda: HCase(2, 2, 4.0, 0.05).device(2, 10, 5, 5, options=BIT), L.AFQ_EINVAL)


def test_m_57_configures_with_the_bit():
    c = case_of(57)
    p64, px = c.path64(5, 1), c.path_ext(5, 1)
    dev = c.device(1, 5, options=BIT)
    try:
        check("trial G", dev.get(L.F_THERMAL_G), p64.G, px.G)
        check("trial M0", dev.get(L.F_THERMAL_M0), p64.M0, px.M0, relative=True)
    finally:
        dev.close()


# ---- 9: reset and the device's stream at M = 57
def test_reset_and_philox_at_57():
    """afq_thermal_reset and then the same fields reproduce a 4-slice path bit for bit; xi = None twice with one seed
    gives equal bits, and the fields read back reproduce the run."""
    c = case_of(57)
    nw = 2
    dev = c.device(nw, 5, options=BIT)
    try:
        M00 = dev.get(L.F_THERMAL_M0)
        runs = []
        for mode in ("draw", "draw", "feed", "feed"):
            dev.rng_seed(1234, 0)
            dev.thermal_reset()
            dev.set(L.F_THERMAL_M0, M00)              # (a reset leaves M0 where the last path ended, as the reference does)
            assert dev.thermal_state() == (0, 0, 0, 2)
            numpy.testing.assert_array_equal(dev.get(L.F_WEIGHT), numpy.ones(nw))
            out, fields = [], []
            for ts in range(4):
                xi = None if mode == "draw" else runs[0][1][ts]
                fields.append(dev.thermal_propagate_continuous(xi, fetch_fields=True))
                out.append([dev.get(f) for f in WALKER_FIELDS])
            runs.append((out, fields))
        f = numpy.array(runs[0][1])
        assert len(numpy.unique(f)) == f.size
        for other in runs[1:]:
            numpy.testing.assert_array_equal(numpy.array(other[1]), f)
            for a, b in zip(runs[0][0], other[0]):
                for x, y in zip(a, b):
                    numpy.testing.assert_array_equal(x, y)
    finally:
        dev.close()
