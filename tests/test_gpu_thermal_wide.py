"""The wide route of the complex thermal walkers (AFQ_THERMAL_WIDE, walkers: {wide_basis: True}): one complex matrix in
LDS, two columns per lane, everything else in the work-group's scratch in device memory -- thermal_cgreens_wide_kernel
(thermal_wide.h) and the two wide slice kernels of k_thermal_cplx.hip -- which carries the electron gas to the shells of
81 and 93 plane waves and the Hubbard model with continuous fields to 95 sites.

The rule is the one of every thermal test (tests/itcf_ref_ext.py): the device lies within 100 max(err_ref, 1e-15) of the
numpy.clongdouble restatement on the scale max(1, max |quantity|), err_ref the reference's own distance from it where a
fixture holds the reference's record and the fp64 restatement's elsewhere; determinants, M0 and weights relative.  Every
comparison prints err_ref, device error, bound and fraction; THERMAL_WIDE_PRECISION_OUT=<file> writes them as the
table of profiles/thermal_wide_precision.md.  The extended restatements of the fixture cases at M = 81 and 93 take a
minute and more, so they are read from the three *_ext.npz files of tests/thermal_wide_cases.py (make_thermal_wide_ext.py; the CPU tests
recompute a part of it).

Shapes of the engine's edges, on Hubbard chains 1 x M: 33 (every column in the low half of the lanes), 64 (the last
with an empty second column), 65 (the first with one), 80 (five MFMA tiles), 81, the library's largest M (95) and that
M + 1 refused.  Every handle here carries the bit unless the test sets two routes side by side."""
import os
import types

import numpy
import pytest

from pauxy_amd import _lib as L
from tests import thermal_hubbard_cont_cases as C
from tests import thermal_ueg_ref as ur
from tests import thermal_ueg_ref_ext as ue
from tests import thermal_wide_cases as W
from tests.thermal_ueg_cases import Case

pytestmark = pytest.mark.gpu

BIT = getattr(L, "THERMAL_WIDE", 32)                     # (a library without the option refuses the bit: every test fails)
STREAMED_BIT = L.THERMAL_STREAMED_GREENS
WIDE = {"thermal_cgreens_wide_kernel", "thermal_cslice_wide_kernel", "thermal_cslice_dense_wide_kernel"}
OLD = {"thermal_cgreens_kernel", "thermal_cgreens_streamed_kernel", "thermal_cslice_kernel", "thermal_cslice_dense_kernel"}
STATE = (L.F_THERMAL_G, L.F_THERMAL_STACK, L.F_THERMAL_RIGHT, L.F_THERMAL_M0, L.F_WEIGHT)

_MEASURED, _GROUP, _ROUTES = [], [""], []


def max_basis():
    return int(L.load().afq_thermal_wide_max_basis())


def check(label, got, ref, want_ext, relative=False, factor=1.0):
    """device within factor x bound(err_ref) of the extended result; err_ref from `ref`."""
    if relative:
        err_ref, err_dev = ue.rerr(ref, want_ext), ue.rerr(got, want_ext)
    else:
        scale = max(1.0, float(numpy.max(numpy.abs(ue.ext(want_ext)))))
        err_ref, err_dev = ue.gerr(ref, want_ext, scale), ue.gerr(got, want_ext, scale)
    bnd = factor * ue.bound(err_ref)
    print("%s: err_ref %.3e device %.3e bound %.3e fraction %.3f" % (label, err_ref, err_dev, bnd, err_dev / bnd))
    _MEASURED.append((_GROUP[0], label, err_ref, err_dev, bnd))
    assert numpy.all(numpy.isfinite(numpy.asarray(got, dtype=complex))), label
    assert err_dev <= bnd, (label, err_ref, err_dev, bnd)


def check_weights(label, got, ref, want_ext):
    """Weights relative where the extended restatement's walker lives; a killed walker's weight is 0 exactly."""
    want = numpy.asarray(want_ext)
    alive = want > 0
    assert numpy.all(numpy.asarray(got)[~alive] == 0) and numpy.all(numpy.asarray(ref)[~alive] == 0), label
    if numpy.any(alive):
        check(label, numpy.asarray(got)[alive], numpy.asarray(ref)[alive], want[alive], relative=True)


@pytest.fixture(autouse=True)
def _group(request):
    _GROUP[0] = request.node.name
    yield


@pytest.fixture(scope="module", autouse=True)
def precision_table():
    yield
    out = os.environ.get("THERMAL_WIDE_PRECISION_OUT")
    if not out or not _MEASURED:
        return
    lines = ["| test | comparison | err_ref | device | bound | fraction |", "|---|---|---|---|---|---|"]
    worst = {}
    for group, label, err_ref, err_dev, bnd in _MEASURED:
        words = label.split()
        key = (group, words[2] if words[0] == "slice" else words[0])
        if key not in worst or err_dev / bnd > worst[key][2] / worst[key][3]:
            worst[key] = (label, err_ref, err_dev, bnd)
    for (group, _), (label, err_ref, err_dev, bnd) in worst.items():
        lines.append("| %s | %s | %.2e | %.2e | %.2e | %.3f |" % (group, label, err_ref, err_dev, bnd, err_dev / bnd))
    lines += ["", "Largest fraction over every comparison of the module: %.3f." % max(e / b for _, _, _, e, b in _MEASURED), ""]
    if _ROUTES:
        lines += ["The wide and the streamed engine side by side on the same bins (largest |difference| per quantity; right",
                  "and the bins are asserted bit-equal, G and det are held to the rule):", "",
                  "| test | quantity | largest difference |", "|---|---|---|"]
        largest = {}
        for group, quantity, diff in _ROUTES:
            largest[group, quantity] = max(largest.get((group, quantity), 0.0), diff)
        lines += ["| %s | %s | %.2e |" % (g, q, v) for (g, q), v in largest.items()] + [""]
    with open(out, "w") as f:
        f.write("\n".join(lines))


def refused(fn, code=None):
    with pytest.raises(L.AfqError) as e:
        fn()
    assert e.value.code == (L.AFQ_EUNSUPPORTED if code is None else code), e.value
    return str(e.value)


def traced(dev):
    return set(dev.launch_trace_get())


_CHAINS = {}


def chain(M, Lts=4):
    if (M, Lts) not in _CHAINS:
        _CHAINS[M, Lts] = C.Chain(M, L=Lts)
    return _CHAINS[M, Lts]


def complex_stack(M, nw, nbins, stack_size, seed, spread=20.0):
    """thermal_ueg_cases.Case.random_stack for any M: complex bins of graded scales."""
    return Case.random_stack(types.SimpleNamespace(M=M, dt=0.05), nw, nbins, stack_size, seed, spread)


# ---- 1: the engine's edges: G and det G alone, on uploaded bins of Hubbard chains
def greens_case(M, nbins, stack_size, slice_ixs, nw=1, seed=5, twice=False):
    stack = complex_stack(M, nw, nbins, stack_size, seed)
    dev = chain(M, nbins * stack_size).device(stack_size, nw, BIT)
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
            tag = "M=%d nbins=%d ss=%d slice_ix=%d" % (M, nbins, stack_size, slice_ix)
            for w in range(nw):                                 # every walker under the rule by itself
                check("G walker %d %s" % (w, tag), G[w], G64[w], Gx[w])
                check("det walker %d %s" % (w, tag), det[w], ur.Kit64.det(G64[w]), ue.det(Gx[w]), relative=True)
            if twice:
                dev.thermal_greens(slice_ix)
                numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_G), G)
                numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_DET), det)
    finally:
        dev.close()


@pytest.mark.parametrize("nbins", [1, 2, 5])
@pytest.mark.parametrize("M", [33, 64, 65, 80, 81, "max"])
def test_wide_greens_and_determinant_on_chains(M, nbins):
    """nbins = 1: no chain product, T goes from the first QR straight to the closing solve."""
    greens_case(max_basis() if M == "max" else M, nbins, 2, [0])


def test_wide_greens_every_starting_slice_at_65():
    """Every slice_ix from 0 to L: the rotation of `first`, and the final one (the chain starts at bin 0)."""
    greens_case(65, 5, 2, list(range(0, 11)))


@pytest.mark.parametrize("M", [65, "max"])
def test_wide_greens_hardest_bins(M):
    """4 bins of 20 slices whose one-body exponents spread over 20 / dt: a bin's condition number is above 1e7, the
    graded scales span the columns of both halves of the lanes."""
    M = max_basis() if M == "max" else M
    cond = numpy.linalg.cond(complex_stack(M, 1, 1, 20, 5)[0, 0, 0])
    print("condition of a bin: %.3e" % cond)
    assert cond > 1e7
    greens_case(M, 4, 20, [0, 80])


@pytest.mark.parametrize("M,nw", [(33, 9), (81, 5)])
def test_wide_scratch_is_per_work_group(M, nw):
    """Distinct walkers in one launch, each under the rule: work-groups that share or overrun a scratch buffer fail
    here.  The same call twice gives the same bits."""
    greens_case(M, 2, 2, [0], nw=nw, twice=True)


def test_the_largest_basis_runs_a_path_and_one_more_is_refused_with_the_numbers():
    """1 x 95 through two slices of afq_thermal_propagate_continuous against the restatement; 1 x 96 is refused naming
    M, the wide Green's kernel, its bytes and the bound.  The bytes are the header's formula, not the library's."""
    M = max_basis()
    assert 16 * (M * (M | 1) + 1152) + 512 <= 160 * 1024 < 16 * ((M + 1) * ((M + 1) | 1) + 1152) + 512
    assert M >= 93
    path_against_restatement(C.Chain(M, L=2), 1, 1, 2, 12, "M=%d" % M)
    text = refused(lambda: C.Chain(M + 1, L=2).device(2, 1, BIT))
    lds = 16 * ((M + 1) * ((M + 1) | 1) + 1152) + 512
    assert "M = %d" % (M + 1) in text and "thermal_cgreens_wide_kernel" in text and str(lds) in text
    assert "M <= %d" % M in text and "wide_basis" in text


# ---- 2: whole slices against the restatement
def path_against_restatement(ch, stack_size, nw, nslice, seed, tag):
    rng = numpy.random.RandomState(seed)
    p64, px = ch.path(stack_size, nw, False), ch.path(stack_size, nw, True)
    dev = ch.device(stack_size, nw, BIT)
    try:
        check("trial G " + tag, dev.get(L.F_THERMAL_G), p64.G, px.G)
        check("trial M0 " + tag, dev.get(L.F_THERMAL_M0), p64.M0, px.M0, relative=True)
        for ts in range(nslice):
            xi = rng.normal(size=(nw, ch.M))
            xb64, cmf64, cfb64 = p64.step(xi)
            xbx, cmfx, cfbx = px.step(xi)
            dev.thermal_propagate_continuous(xi)
            t = "slice %d %%s %s" % (ts + 1, tag)
            check(t % "xbar", dev.get(L.F_XBAR), xb64, xbx)
            check(t % "cmf", dev.get(L.F_CMF), cmf64, cmfx)
            check(t % "cfb", dev.get(L.F_CFB), cfb64, cfbx)
            check(t % "right", dev.get(L.F_THERMAL_RIGHT), p64.right, px.right)
            check(t % "bins", dev.get(L.F_THERMAL_STACK), p64.stack, px.stack)
            check(t % "G", dev.get(L.F_THERMAL_G), p64.G, px.G)
            check(t % "M0", dev.get(L.F_THERMAL_M0), p64.M0, px.M0, relative=True)
            check_weights(t % "weight", dev.get(L.F_WEIGHT), p64.weight, px.weight)
        assert int(dev.counters()[0]) == px.nclip == p64.nclip
        return dev.thermal_energy(), p64.energy(), px.energy()
    finally:
        dev.close()


@pytest.mark.parametrize("M", [33, 65])
def test_wide_path_on_a_chain(M):
    """stack_size 2 of 4 slices: both branches of the in-bin counter of the dense wide slice kernel, 2 walkers; the
    energies and nav of the last G."""
    ch = chain(M)
    (E, nav), (E64, nav64), (Ex, navx) = path_against_restatement(ch, 2, 2, 4, 30 + M, "M=%d" % M)
    scale = float(numpy.max(numpy.sum(numpy.abs(numpy.asarray(ch.system.H1)[0]), axis=0))) + ch.system.U * M
    check("energy", E, numpy.asarray(E64).real, numpy.asarray(Ex).real, factor=scale)
    check("nav", nav, numpy.asarray(nav64).real, numpy.asarray(navx).real, factor=M)


# ---- 3: wide against what exists, where both run
def note_routes(quantity, a, b):
    _ROUTES.append((_GROUP[0], quantity, float(numpy.max(numpy.abs(numpy.asarray(a) - numpy.asarray(b))))))


def side_by_side(make_device, K, nslice, nw, seed):
    """The same fields through a wide and a streamed handle; before every slice the wide handle is given the streamed
    handle's G, so both slice kernels see the same P: right and the bins bit for bit after every slice, G and det under
    the rule against the restatement of the Green's function of those very bins, their distance from the streamed
    engine's recorded."""
    rng = numpy.random.RandomState(seed)
    wide, old = make_device(BIT), make_device(STREAMED_BIT)
    try:
        wide.launch_trace(True)
        old.launch_trace(True)
        for ts in range(nslice):
            xi = rng.normal(size=(nw, K))
            wide.set(L.F_THERMAL_G, old.get(L.F_THERMAL_G))
            wide.thermal_propagate_continuous(xi)
            old.thermal_propagate_continuous(xi)
            numpy.testing.assert_array_equal(wide.get(L.F_XBAR), old.get(L.F_XBAR))
            numpy.testing.assert_array_equal(wide.get(L.F_THERMAL_RIGHT), old.get(L.F_THERMAL_RIGHT))
            stack = old.get(L.F_THERMAL_STACK)
            numpy.testing.assert_array_equal(wide.get(L.F_THERMAL_STACK), stack)
            M, nbins = stack.shape[-1], stack.shape[1]
            bins = [stack[:, b].reshape(nw * 2, M, M) for b in range(nbins)]
            G = wide.get(L.F_THERMAL_G)
            G64, Gx = ur.strat_greens(bins).reshape(G.shape), ue.strat_greens(bins).reshape(G.shape)
            check("slice %d G" % (ts + 1), G, G64, Gx)
            check("slice %d det" % (ts + 1), wide.get(L.F_THERMAL_DET), ur.Kit64.det(G64), ue.det(Gx), relative=True)
            note_routes("G", G, old.get(L.F_THERMAL_G))
            note_routes("det (relative)", wide.get(L.F_THERMAL_DET) / old.get(L.F_THERMAL_DET), 1.0)
        assert traced(wide) & (WIDE | OLD) <= WIDE and len(traced(wide) & WIDE) == 2
        assert not traced(old) & WIDE
    finally:
        wide.close()
        old.close()


@pytest.mark.parametrize("M,ecut", [(19, 1.0), (57, 2.5)])
def test_wide_slice_has_the_bits_of_the_present_ueg_slice_kernel(M, ecut):
    """thermal_cslice_wide_kernel against thermal_cslice_kernel over a bin and into the next (stack_size 2, 3 slices:
    the in-bin counter 0, 1, 0)."""
    c = Case(ecut, 2)
    assert c.M == M
    side_by_side(lambda options: c.device(2, 2, options=options), c.K, 3, 2, 7)


def test_wide_slice_has_the_bits_of_the_present_dense_slice_kernel():
    """thermal_cslice_dense_wide_kernel against thermal_cslice_dense_kernel on the 6 x 6 lattice of the fixture."""
    side_by_side(lambda options: C.device('a6_', 2, stack_size=2, options=options), 36, 3, 2, 8)


# ---- 4: the population
def whole_path(dev, xis):
    out = []
    for xi in xis:
        dev.thermal_propagate_continuous(xi)
        out.append([dev.get(f) for f in STATE])
    out.append(list(dev.thermal_energy()))
    return out


def same_bits(a, b, walkers=slice(None)):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            numpy.testing.assert_array_equal(u[walkers], v)


def test_same_bits_on_repeat_and_with_1_and_65_walkers():
    """A whole path at M = 65 (2 bins): the same bits after a reset with M0 put back; walker 40 of 65 walkers that all
    get the one walker's fields has the one walker's bits (more work-groups than one wave of them: the grid position
    does not enter)."""
    ch = chain(65)
    xis = numpy.random.RandomState(9).normal(size=(4, 1, 65))
    dev = ch.device(2, 1, BIT)
    try:
        M00 = dev.get(L.F_THERMAL_M0)
        first = whole_path(dev, xis)
        dev.thermal_reset()
        dev.set(L.F_THERMAL_M0, M00)
        assert dev.thermal_state() == (0, 0, 0, 2)
        same_bits(first, whole_path(dev, xis))
    finally:
        dev.close()
    dev = ch.device(2, 65, BIT)
    try:
        same_bits(whole_path(dev, numpy.repeat(xis, 65, axis=1)), first, walkers=slice(40, 41))
    finally:
        dev.close()


def test_a_dead_walker_still_draws_fields_and_moves():
    ch = chain(65)
    rng = numpy.random.RandomState(5)
    p64, px = ch.path(2, 3, False), ch.path(2, 3, True)
    dev = ch.device(2, 3, BIT)
    try:
        w = dev.get(L.F_WEIGHT)
        w[1] = 0.0
        dev.set(L.F_WEIGHT, w)
        p64.weight[1] = px.weight[1] = 0
        for ts in range(2):
            xi = rng.normal(size=(3, 65))
            p64.step(xi)
            px.step(xi)
            used = dev.thermal_propagate_continuous(xi, fetch_fields=True)
            numpy.testing.assert_array_equal(used, xi)
            check("slice %d G" % (ts + 1), dev.get(L.F_THERMAL_G), p64.G, px.G)
            check("slice %d bins" % (ts + 1), dev.get(L.F_THERMAL_STACK), p64.stack, px.stack)
            check("slice %d M0" % (ts + 1), dev.get(L.F_THERMAL_M0), p64.M0, px.M0, relative=True)
            got = dev.get(L.F_WEIGHT)
            assert got[1] == 0.0 and got[0] > 0 and got[2] > 0
            assert numpy.max(numpy.abs(dev.get(L.F_XBAR)[1])) > 0
    finally:
        dev.close()


def test_kill_branches_of_the_weight_update():
    """As test_gpu_thermal_hubbard_cont.py's, on a wide handle.  Walker 1: M0 huge, magn overflows: weight 0, M0 kept.
    Walker 2: the sign of one M0 flipped (cos = -1): weight 0, M0 updated.  Walker 3: M0 not a number: weight 0, M0
    kept.  Walker 4: the other bin scaled by 1e80: det G_s = 0 in fp64 (the LU's zero pivot leaves by the uniform
    exit), weight 0, M0 kept.  Walker 0 untouched."""
    ch = C.Chain(9, L=4)
    dev = ch.device(2, 5, BIT)
    try:
        xi = numpy.random.RandomState(3).normal(size=(5, 9))
        M0 = dev.get(L.F_THERMAL_M0)
        huge = numpy.array([1e200 + 0j, 1e200 + 0j])
        M0[1] = huge
        M0[2, 0] = -M0[2, 0]
        M0[3, 1] = numpy.nan
        dev.set(L.F_THERMAL_M0, M0)
        stack = dev.get(L.F_THERMAL_STACK)
        stack[4, 1] *= 1e80
        dev.set(L.F_THERMAL_STACK, stack)
        dev.thermal_propagate_continuous(xi)
        w, M1, det = dev.get(L.F_WEIGHT), dev.get(L.F_THERMAL_M0), dev.get(L.F_THERMAL_DET)
        assert w[0] > 0 and w[1] == 0.0 and w[2] == 0.0 and w[3] == 0.0 and w[4] == 0.0
        numpy.testing.assert_array_equal(M1[1], huge)
        assert numpy.isnan(M1[3, 1]) and M1[3, 0] == M0[3, 0]
        numpy.testing.assert_array_equal(M1[0], det[0])
        numpy.testing.assert_array_equal(M1[2], det[2])
        assert numpy.all(det[4] == 0) and numpy.all(numpy.abs(det[:4]) > 0)
        numpy.testing.assert_array_equal(M1[4], M0[4])
    finally:
        dev.close()


def test_reset_carries_m0_into_the_second_path():
    ch = chain(65, 2)
    rng = numpy.random.RandomState(21)
    p64, px = ch.path(1, 2, False), ch.path(1, 2, True)
    dev = ch.device(1, 2, BIT)
    try:
        for path in range(2):
            for ts in range(2):
                xi = rng.normal(size=(2, 65))
                p64.step(xi)
                px.step(xi)
                dev.thermal_propagate_continuous(xi)
                check("path %d slice %d M0" % (path, ts + 1), dev.get(L.F_THERMAL_M0), p64.M0, px.M0, relative=True)
                check_weights("path %d slice %d weight" % (path, ts + 1), dev.get(L.F_WEIGHT), p64.weight, px.weight)
            M1 = dev.get(L.F_THERMAL_M0)
            dev.thermal_reset()
            p64.reset()
            px.reset()
            numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_M0), M1)
            assert numpy.all(dev.get(L.F_WEIGHT) == 1.0) and dev.thermal_state() == (0, 0, 0, 2)
            check("path %d trial G again" % path, dev.get(L.F_THERMAL_G), p64.G, px.G)
    finally:
        dev.close()


def test_comb_copy_and_pack_of_a_wide_population():
    """The comb clones G, the bins, right and M0 of its parents bit for bit; afq_walkers_copy and pack / unpack carry
    the same four and the weight."""
    from tests.test_gpu_pair_branch import DeviceBuffer
    ch = chain(65)
    dev = ch.device(2, 4, BIT)
    try:
        dev.thermal_propagate_continuous(numpy.random.RandomState(2).normal(size=(4, 65)))
        dev.set(L.F_WEIGHT, numpy.array([2.2, 1e-3, 0.9, 0.9]))
        before = [dev.get(f) for f in STATE[:4]]
        pix, total = dev.popcontrol_comb(0.37, 4)
        assert list(pix) == [2, 0, 1, 1] and abs(total - 4.001) < 1e-12       # teeth (k + 0.37) 4.001 / 4
        want = [b.copy() for b in before]
        for cl, kl in zip(numpy.where(pix > 1)[0], numpy.where(pix == 0)[0]):
            for x, b in zip(want, before):
                x[kl] = b[cl]
        for x, f in zip(want, STATE[:4]):
            numpy.testing.assert_array_equal(dev.get(f), x)
        dev.thermal_propagate_continuous(numpy.random.RandomState(3).normal(size=(4, 65)))
        state = [dev.get(f) for f in STATE]
        dev.copy_walker(2, 3)
        buf = DeviceBuffer(dev, dev.pack_bytes())
        dev.pack(0, buf.ptr.value)
        dev.unpack(1, buf.ptr.value)
        dev.sync()
        buf.free()
        for x, f in zip(state, STATE):
            got = dev.get(f)
            numpy.testing.assert_array_equal(got[3], x[2])
            numpy.testing.assert_array_equal(got[1], x[0])
            numpy.testing.assert_array_equal(got[[0, 2]], x[[0, 2]])
    finally:
        dev.close()


def test_device_philox_fields():
    """xi = None twice with one seed gives equal bits, and the fields read back reproduce the run when fed."""
    ch = chain(65)
    dev = ch.device(2, 2, BIT)
    try:
        M00 = dev.get(L.F_THERMAL_M0)
        runs = []
        for mode in ("draw", "draw", "feed"):
            dev.rng_seed(1234, 0)
            dev.thermal_reset()
            dev.set(L.F_THERMAL_M0, M00)
            out, fields = [], []
            for ts in range(2):
                xi = None if mode == "draw" else runs[0][1][ts]
                fields.append(dev.thermal_propagate_continuous(xi, fetch_fields=True))
                out.append([dev.get(f) for f in STATE])
            runs.append((out, fields))
        f = numpy.array(runs[0][1])
        assert len(numpy.unique(f)) == f.size
        for other in runs[1:]:
            numpy.testing.assert_array_equal(numpy.array(other[1]), f)
            same_bits(runs[0][0], other[0])
    finally:
        dev.close()


# ---- 5: the estimators of a wide handle
@pytest.mark.parametrize("kind,M", [("dense", 65), ("diag", 81)])
def test_one_rdm_and_two_rdm_on_a_wide_handle(kind, M):
    """afq_thermal_estimates without AVERAGE_GF on uploaded bins: cols are afq_thermal_greens + afq_thermal_energy bit
    for bit, the G it leaves is under the rule, one_rdm = sum_w weight_w Re G_w and (UEG) two_rdm =
    sum_w weight_w Re two_rdm[P_w] within nw eps sum |terms| per element of numpy's sums of the device's own per-walker
    values, one walker of weight zero among them (the measure of tests/test_gpu_thermal_obs.py); AVERAGE_GF is refused
    by name."""
    nw, nbins, ss = 3, 2, 2
    ueg = kind == "diag"
    if ueg:
        c = W.ueg_case(M)
        stack = c.random_stack(nw, nbins, ss, 5)
        dev = c.device(nw, ss, options=BIT, L=nbins * ss)
    else:
        stack = complex_stack(M, nw, nbins, ss, 5)
        dev = chain(M, nbins * ss).device(ss, nw, BIT)
    try:
        dev.set(L.F_THERMAL_STACK, stack)
        weights = numpy.array([0.7, 0.0, 1.3])
        dev.set(L.F_WEIGHT, weights)
        dev.thermal_greens(0)
        E, nav = dev.thermal_energy()
        res = dev.thermal_estimates(one_rdm=True, two_rdm=ueg)
        numpy.testing.assert_array_equal(res['cols'], numpy.concatenate([E, nav[:, None]], axis=1))
        G = dev.get(L.F_THERMAL_G)
        bins = [stack[:, b].reshape(nw * 2, M, M) for b in ur.chain_order(0, ss, nbins)]
        check("G the call leaves", G, ur.strat_greens(bins).reshape(G.shape), ue.strat_greens(bins).reshape(G.shape))
        terms = weights[:, None, None, None] * G.real
        bound = nw * 2.0 ** -52 * numpy.sum(numpy.abs(terms), axis=0)
        assert numpy.all(numpy.abs(res['one_rdm'] - numpy.sum(terms, axis=0)) <= bound)
        if ueg:
            P = numpy.eye(M)[None, None] - numpy.swapaxes(G, -1, -2)
            _, two = dev.ueg_pair_sums(P)
            terms = weights[:, None, None, None] * two.real
            bound = nw * 2.0 ** -52 * numpy.sum(numpy.abs(terms), axis=0)
            assert numpy.all(numpy.abs(res['two_rdm'] - numpy.sum(terms, axis=0)) <= bound)
            assert numpy.max(numpy.abs(res['two_rdm'])) > 0
        text = refused(lambda: dev.thermal_estimates(average_gf=True))
        assert "average_gf" in text and "wide_basis" in text
    finally:
        dev.close()


# ---- 6: refusals, the trace, the neighbours
def test_refusals_of_the_bit():
    """The real walkers refuse the bit by name; the two bits together are AFQ_EINVAL on both continuous entry points;
    bit 64 stays unknown; M above the bound on the UEG entry point names the numbers."""
    from tests.thermal_cases import Case as HCase
    text = refused(lambda: HCase(2, 2, 4.0, 0.05).device(2, 10, 5, 5, options=BIT), L.AFQ_EINVAL)
    assert "afq_thermal_configure: " in text and "wide_basis" in text and "unknown" not in text
    both = BIT | STREAMED_BIT
    for fn in (lambda o: chain(9).device(2, 1, o), lambda o: W.ueg_case(7).device(1, 5, options=o)):
        text = refused(lambda: fn(both), L.AFQ_EINVAL)
        assert "wide_basis" in text and "streamed_greens" in text
        assert "unknown option bits" in refused(lambda: fn(64), L.AFQ_EINVAL)
        assert "unknown option bits" in refused(lambda: fn(64 | BIT), L.AFQ_EINVAL)
    c = Case(5.0, 2)
    assert c.M > max_basis()
    text = refused(lambda: c.device(1, 5, options=BIT))
    lds = 16 * (c.M * (c.M | 1) + 1152) + 512
    assert "M = %d plane waves" % c.M in text and "thermal_cgreens_wide_kernel" in text and str(lds) in text
    assert "M <= %d" % max_basis() in text and "163840" in text


def test_launch_trace_names_the_three_wide_kernels_and_none_of_the_old():
    names = set()
    for make, K in ((lambda: chain(33).device(2, 1, BIT), 33), (lambda: W.ueg_case(19).device(1, 5, options=BIT), None)):
        dev = make()
        try:
            dev.launch_trace(True)
            dev.thermal_reset()
            dev.thermal_propagate_continuous(numpy.random.RandomState(1).normal(size=(1, K or W.ueg_case(19).K)))
            dev.thermal_greens(1)
            dev.thermal_estimates(one_rdm=True)
            names |= traced(dev)
        finally:
            dev.close()
    assert WIDE <= names and not names & OLD, names


def test_neighbours_without_the_bit_are_what_they_were():
    """M = 33 without a bit launches the resident kernels, M = 57 with STREAMED_GREENS the streamed one, and M = 81
    with STREAMED_GREENS alone is refused in the words tests/test_gpu_thermal_ueg_streamed.py pins."""
    for M, options, greens in ((33, 0, "thermal_cgreens_kernel"), (57, STREAMED_BIT, "thermal_cgreens_streamed_kernel")):
        c = W.ueg_case(M)
        dev = c.device(1, 5, options=options)
        try:
            dev.launch_trace(True)
            dev.thermal_propagate_continuous(numpy.random.RandomState(1).normal(size=(1, c.K)))
            assert traced(dev) & (WIDE | OLD) == {greens, "thermal_cslice_kernel"}
        finally:
            dev.close()
    text = refused(lambda: W.ueg_case(81).device(1, 5, options=STREAMED_BIT))
    assert "81" in text and "57" in text and "slice kernel" in text and "thermal_cslice_kernel" in text
    assert "wide" not in text


# ---- 7: the fixture cases at M = 81 and 93, and on 8 x 8 and 1 x 65
@pytest.mark.parametrize("name,pre", [("thermal_ueg81.npz", "a6_"), ("thermal_ueg93.npz", "a7_")])
def test_ueg_fixture_case_slice_by_slice(name, pre):
    """The recorded fields of the reference's walker through afq_thermal_propagate_continuous: xbar, cmf, cfb, M0 and
    the weight after every slice, G at the slices the fixture holds, under the rule with err_ref the REFERENCE's own
    distance from the stored extended restatement; the bins and right of every slice are held by the tests above (the
    bits of the present kernel to M = 57, the rule on chains to M = 95); the clip count; the final energies and nav."""
    d, x = W.golden(name), W.stored_ext()
    c = W.case_of_fixture(d, pre)
    ss, M = int(d[pre + 'stack_size']), c.M
    stored = {int(n): i for i, n in enumerate(d[pre + 'G_slices'])}
    dev = c.device(1, ss, options=BIT)
    try:
        check("trial M0", dev.get(L.F_THERMAL_M0)[0], d[pre + 'M00'], W.joined(x, pre + 'M00'), relative=True)
        for ts in range(c.L):
            used = dev.thermal_propagate_continuous(d[pre + 'xi'][ts][None], fetch_fields=True)
            numpy.testing.assert_array_equal(used[0], d[pre + 'xi'][ts])
            tag = "slice %d " % (ts + 1)
            check(tag + "xbar", dev.get(L.F_XBAR)[0], d[pre + 'xbar'][ts], W.joined(x, pre + 'xbar')[ts])
            check(tag + "cmf", dev.get(L.F_CMF)[0], d[pre + 'cmf'][ts], W.joined(x, pre + 'cmf')[ts])
            check(tag + "cfb", dev.get(L.F_CFB)[0], d[pre + 'cfb'][ts], W.joined(x, pre + 'cfb')[ts])
            check(tag + "M0", dev.get(L.F_THERMAL_M0)[0], d[pre + 'M0'][ts], W.joined(x, pre + 'M0')[ts], relative=True)
            check(tag + "weight", dev.get(L.F_WEIGHT)[0], d[pre + 'weight'][ts], W.joined(x, pre + 'weight')[ts], relative=True)
            if ts + 1 in stored:
                i = stored[ts + 1]
                check(tag + "G", dev.get(L.F_THERMAL_G)[0], d[pre + 'G'][i], W.joined(x, pre + 'G')[i])
        assert int(dev.counters()[0]) == int(d[pre + 'nclip']) == 0
        E, nav = dev.thermal_energy()
        scale = float(numpy.max(numpy.abs(c.ops.H1diag))) * M + float(numpy.sum(c.ops.vqvec)) / c.system.vol * M
        check("energy", E[0], d[pre + 'energy'].real, W.joined(x, pre + 'energy').real, factor=scale)
        check("nav", nav[0], complex(d[pre + 'nav']).real, W.joined(x, pre + 'nav').real, factor=M)
    finally:
        dev.close()


@pytest.mark.parametrize("k", [8, 9])
def test_hubbard_fixture_case_slice_by_slice(k):
    """8 x 8 (M = 64) and 1 x 65 from thermal_hubbard_cont_wide.npz, as the UEG cases: the reference's record against the
    stored extended restatement; G behind the last slice."""
    d, x = W.golden("thermal_hubbard_cont_wide.npz"), W.stored_ext()
    pre = 'h%d_' % k
    a = 'a%d_' % k
    dev = W.hubbard_device(d, a, 1, BIT)
    M = int(d[a + 'nx']) * int(d[a + 'ny'])
    try:
        check("trial M0", dev.get(L.F_THERMAL_M0)[0], d[a + 'M00'], W.joined(x, pre + 'M00'), relative=True)
        for ts in range(10):
            dev.thermal_propagate_continuous(d[a + 'xi'][ts][None])
            tag = "slice %d " % (ts + 1)
            check(tag + "xbar", dev.get(L.F_XBAR)[0], d[a + 'xbar'][ts], W.joined(x, pre + 'xbar')[ts])
            check(tag + "cmf", dev.get(L.F_CMF)[0], d[a + 'cmf'][ts], W.joined(x, pre + 'cmf')[ts])
            check(tag + "cfb", dev.get(L.F_CFB)[0], d[a + 'cfb'][ts], W.joined(x, pre + 'cfb')[ts])
            check(tag + "M0", dev.get(L.F_THERMAL_M0)[0], d[a + 'M0'][ts], W.joined(x, pre + 'M0')[ts], relative=True)
            check(tag + "weight", dev.get(L.F_WEIGHT)[0], d[a + 'weight'][ts], W.joined(x, pre + 'weight')[ts], relative=True)
        check("last G", dev.get(L.F_THERMAL_G)[0], d[a + 'G_last'], W.joined(x, pre + 'G_last'))
        assert int(dev.counters()[0]) == int(d[a + 'nclip'])
        E, nav = dev.thermal_energy()
        H1 = numpy.asarray(W.hubbard_system(d, a).H1)
        scale = float(numpy.max(numpy.sum(numpy.abs(H1[0]), axis=0))) + float(d[a + 'U']) * M
        check("energy", E[0], d[a + 'energy'].real, W.joined(x, pre + 'energy').real, factor=scale)
        check("nav", nav[0], complex(d[a + 'nav']).real, W.joined(x, pre + 'nav').real, factor=M)
    finally:
        dev.close()


# ---- 8: the drivers, through the Python classes
def clones_are_bit_for_bit(parents, states):
    nclone = 0
    for parent, (before, after) in zip(parents, states):
        want = [b.copy() for b in before]
        for cl, kl in zip(numpy.where(parent > 1)[0], numpy.where(parent == 0)[0]):
            for xx, b in zip(want, before):
                xx[kl] = b[cl]
            nclone += 1
        for xx, a in zip(want, after):
            numpy.testing.assert_array_equal(xx, a)
    return nclone


def test_ueg_driver_at_81():
    """ThermalAFQMC with walkers: {stack_size: 5, wide_basis: True} over two paths from the recorded seed: the
    reference's comb parents exactly, its estimator rows and its weights after every slice under the rule against the
    stored extended restatement of the run; a clone carries G, the bins, right and M0 of its parent bit for bit."""
    from tests.test_gpu_thermal_ueg import b_options, run_driver
    d, x = W.golden("thermal_ueg81.npz"), W.stored_ext()
    pre, options = b_options(d, 5)
    options['walkers']['wide_basis'] = True
    rows, header, weights, parents, states, _ = run_driver(options, record_state=True)
    assert header == list(d[pre + 'header'])
    numpy.testing.assert_array_equal(numpy.array(parents), d[pre + 'parent_ix'])
    numpy.testing.assert_array_equal(numpy.array(parents), x[pre + 'parents'])
    gold = d[pre + 'blocks'].real
    assert rows.shape == gold.shape == (3, 12)
    check("rows", rows[:, 1:11], gold[:, 1:11], W.joined(x, pre + 'rx'))
    check("weights", weights, d[pre + 'weights'], W.joined(x, pre + 'wx'), relative=True)
    assert clones_are_bit_for_bit(parents, states) > 0


def test_hubbard_driver_on_8x8():
    """ThermalAFQMC with hubbard_stratonovich: 'continuous' and walkers: {wide_basis: True} on 8 x 8 with 4 walkers:
    parents and the clip count exactly, rows and weights under the rule."""
    from tests.test_gpu_thermal_hubbard_cont import run_driver
    d, x = W.golden("thermal_hubbard_cont_wide.npz"), W.stored_ext()
    pre = 'b2_'
    options = W.hubbard_driver_options(d, pre, wide_basis=True)
    rows, header, weights, parents, nclip, kind = run_driver(options)
    assert kind == 'Continuous' and header == list(d[pre + 'header'])
    numpy.testing.assert_array_equal(numpy.array(parents), d[pre + 'parent_ix'])
    numpy.testing.assert_array_equal(numpy.array(parents), x['hb2_parents'])
    assert nclip == int(d[pre + 'nclip'])
    gold = d[pre + 'blocks'].real
    cols = [0, 1, 2, 3, 4, 5, 6, 9]                    # (EHybrid is 0 and Overlap 1 in every row)
    check("rows", rows[:, 1:11][:, cols], gold[:, 1:11][:, cols], W.joined(x, 'hb2_rx')[:, cols], relative=True)
    ref_w = d[pre + 'weights']
    alive = ref_w > 0
    check("weights", weights[alive], ref_w[alive], W.joined(x, 'hb2_wx')[alive], relative=True)
    assert numpy.all(weights[~alive] == 0)
