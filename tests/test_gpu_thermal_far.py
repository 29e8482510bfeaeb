"""The far route of the complex thermal walkers (AFQ_THERMAL_FAR, walkers: {far_basis: True}): the wide route with no
matrix in LDS -- thermal_cgreens_far_kernel (thermal_wide.h: the wide body with W as a fifth buffer of the work-group's
scratch) and the two far slice kernels of k_thermal_cplx.hip -- which carries the electron gas to the shell of 123 plane
waves and the Hubbard model with continuous fields to 128 sites.

1. Where the wide route runs as well the far route gives its bits: G, det, the bins, right, M0, the weights and the clip
   counts compared with ==.
2. Where only the far route runs (M = 123; 8 x 16 = 128 sites; the drivers at M = 123 and on 10 x 10) the rule of every
   thermal test holds (tests/itcf_ref_ext.py): the device lies within 100 max(err_ref, 1e-15) of the stored
   numpy.clongdouble restatement, err_ref the reference's own distance from it; comb parents and clip counts exact,
   clones bit for bit.  Every comparison prints err_ref, device error, bound and fraction; THERMAL_FAR_PRECISION_OUT=<file>
   writes them as the table of profiles/thermal_far_precision.md.
3. Refusals and housekeeping."""
import functools
import os

import numpy
import pytest

from pauxy_amd import _lib as L
from tests import thermal_far_cases as F
from tests import thermal_hubbard_cont_cases as C
from tests import thermal_wide_cases as W
from tests import thermal_ueg_ref_ext as ue

pytestmark = pytest.mark.gpu

FAR = getattr(L, "THERMAL_FAR", 256)                    # (a library without the option refuses the bit: every test fails)
WIDE, STREAMED = L.THERMAL_WIDE, L.THERMAL_STREAMED_GREENS
FAR_KERNELS = {"thermal_cgreens_far_kernel", "thermal_cslice_far_kernel", "thermal_cslice_dense_far_kernel"}
OTHERS = {"thermal_cgreens_kernel", "thermal_cgreens_streamed_kernel", "thermal_cgreens_wide_kernel", "thermal_cslice_kernel",
          "thermal_cslice_dense_kernel", "thermal_cslice_wide_kernel", "thermal_cslice_dense_wide_kernel"}
STATE = (L.F_THERMAL_G, L.F_THERMAL_DET, L.F_THERMAL_STACK, L.F_THERMAL_RIGHT, L.F_THERMAL_M0, L.F_WEIGHT)

_MEASURED, _GROUP = [], [""]


def check(label, got, ref, want_ext, relative=False, factor=1.0):
    """device within factor x bound(err_ref) of the extended result; err_ref from `ref` (the reference's record)."""
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


@pytest.fixture(autouse=True)
def _group(request):
    _GROUP[0] = request.node.name
    yield


@pytest.fixture(scope="module", autouse=True)
def precision_table():
    yield
    out = os.environ.get("THERMAL_FAR_PRECISION_OUT")
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
    with open(out, "w") as f:
        f.write("\n".join(lines))


def refused(fn, code=None):
    with pytest.raises(L.AfqError) as e:
        fn()
    assert e.value.code == (L.AFQ_EUNSUPPORTED if code is None else code), e.value
    return str(e.value)


def traced(dev):
    return set(dev.launch_trace_get())


def far_max():
    return int(L.load().afq_thermal_far_max_basis())


# ---- 1: the bits of the wide route where both run
def complex_stack(M, nw, nbins, stack_size, seed):
    from tests.test_gpu_thermal_wide import complex_stack as make
    return make(M, nw, nbins, stack_size, seed)


@pytest.mark.parametrize("M", [7, 19, 70, 93])
def test_far_greens_has_the_bits_of_the_wide_engine(M):
    """G and det on uploaded bins of a Hubbard chain, 2 walkers, 3 bins of 2 slices, at slice_ix 0 and 3 (as
    wide_greens_digest of tests/test_gpu_thermal_route_bits.py): 7 is one ragged MFMA tile, 19 one full and one ragged,
    70 a lane's second column with the last tile ragged, 93 the largest shell the wide route holds."""
    stack = complex_stack(M, 2, 3, 2, 5)
    got = {}
    for bit in (WIDE, FAR):
        dev = C.Chain(M, L=6).device(2, 2, bit)
        try:
            dev.launch_trace(True)
            dev.set(L.F_THERMAL_STACK, stack)
            out = []
            for s in (0, 3):
                dev.thermal_greens(s)
                out += [dev.get(L.F_THERMAL_G), dev.get(L.F_THERMAL_DET)]
            got[bit] = out
            names = traced(dev) & (FAR_KERNELS | OTHERS)
            assert names == ({"thermal_cgreens_far_kernel"} if bit == FAR else {"thermal_cgreens_wide_kernel"}), names
        finally:
            dev.close()
    assert numpy.all(numpy.isfinite(got[FAR][0])) and numpy.max(numpy.abs(got[FAR][0])) > 0
    for a, b in zip(got[FAR], got[WIDE]):
        numpy.testing.assert_array_equal(a, b)


def path_arrays(dev, xis, K):
    """Every slice's state with xbar, cmf and cfb on a two-walker handle (the given fields for walker 0, a stream of
    RandomState(42) for walker 1), the energies after the last slice, a reset and one more slice; the clip count."""
    rng = numpy.random.RandomState(42)
    nslice = len(xis)
    out = []
    for ts in range(nslice + 1):
        if ts == nslice:
            dev.thermal_reset()
        dev.thermal_propagate_continuous(numpy.array([xis[ts % nslice], rng.normal(size=K)]))
        out += [dev.get(f) for f in STATE + (L.F_XBAR, L.F_CMF, L.F_CFB)]
        if ts == nslice - 1:
            out += list(dev.thermal_energy())
    return out, int(dev.counters()[0])


def same_path_on_both_routes(make_device, xis, K, slice_kernel):
    got = {}
    for bit in (WIDE, FAR):
        dev = make_device(bit)
        try:
            dev.launch_trace(True)
            got[bit] = path_arrays(dev, xis, K)
            if bit == FAR:
                assert traced(dev) & (FAR_KERNELS | OTHERS) == {"thermal_cgreens_far_kernel", slice_kernel}
        finally:
            dev.close()
    assert got[FAR][1] == got[WIDE][1]
    assert len(got[FAR][0]) == len(got[WIDE][0])
    for a, b in zip(got[FAR][0], got[WIDE][0]):
        assert numpy.all(numpy.isfinite(numpy.asarray(a, dtype=complex)))
        numpy.testing.assert_array_equal(a, b)
    return got[FAR]


@pytest.mark.parametrize("pre,M", [('a0_', 7), ('a1_', 7), ('a2_', 19), ('a3_', 33)])
def test_far_ueg_path_has_the_bits_of_the_wide_route(pre, M):
    """Cases of thermal_ueg.npz beside a second walker.  a2: M = 19, two bins of 5 slices.  a0 and a1: M = 7, one bin
    of ten slices and ten bins of one: the product right <- B right on every slice (a0) and the copy that opens a bin
    on every slice (a1), one MFMA tile.  a3: M = 33, five bins of 2 slices -- nine tiles, so the waves' shares of a
    Horner product differ: the case that caught BV read before the barrier behind the last product when that was tried
    (profiles/thermal_far_precision.md; the cases at M = 7 did not).  A missing barrier shows by the waves' timing, so
    that catch is likely, not certain."""
    from tests.test_gpu_thermal_hubbard_cont import ueg_case
    c, ss, xis = ueg_case(pre)
    assert c.M == M
    same_path_on_both_routes(lambda bit: c.device(2, ss, bit), xis, c.K, "thermal_cslice_far_kernel")


@pytest.mark.parametrize("lattice", ["6x6", "8x8"])
def test_far_hubbard_path_has_the_bits_of_the_wide_route(lattice):
    """6 x 6 (case a6 of thermal_hubbard_cont.npz at stack_size 2: the in-bin counter 0, 1, 0 ..) and 8 x 8 (case a8 of
    thermal_hubbard_cont_wide.npz, stack_size 5), four slices each beside a second walker."""
    if lattice == "6x6":
        d = C.golden()
        same_path_on_both_routes(lambda bit: C.device('a6_', 2, stack_size=2, options=bit), d['a6_xi'][:4], 36,
                                 "thermal_cslice_dense_far_kernel")
    else:
        d = W.golden(W.HUBBARD)
        same_path_on_both_routes(lambda bit: W.hubbard_device(d, 'a8_', 2, bit), d['a8_xi'][:4], 64,
                                 "thermal_cslice_dense_far_kernel")


def test_far_ueg_driver_at_81_has_the_bits_of_the_wide_route():
    """The driver run b5 of thermal_ueg81.npz (6 walkers, two paths, a comb event that clones) with far_basis and with
    wide_basis: rows, weights after every slice, parents and the walkers' state around every comb, bit for bit; the
    reference's parents."""
    from tests.test_gpu_thermal_ueg import b_options, run_driver
    d = W.golden("thermal_ueg81.npz")
    runs = {}
    for key in ('wide_basis', 'far_basis'):
        pre, options = b_options(d, 5)
        options['walkers'][key] = True
        runs[key] = run_driver(options, record_state=True)
    far, wide = runs['far_basis'], runs['wide_basis']
    numpy.testing.assert_array_equal(numpy.array(far[3]), d[pre + 'parent_ix'])
    assert numpy.any(numpy.array(far[3]) > 1)
    numpy.testing.assert_array_equal(far[0][:, :11], wide[0][:, :11])           # (the last column is the wall time)
    numpy.testing.assert_array_equal(far[2], wide[2])
    numpy.testing.assert_array_equal(numpy.array(far[3]), numpy.array(wide[3]))
    for (fb, fa), (wb, wa) in zip(far[4], wide[4]):
        for a, b in zip(fb + fa, wb + wa):
            numpy.testing.assert_array_equal(a, b)


# ---- 2: the rule where only the far route runs
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


@functools.lru_cache(maxsize=None)
def bins64(which):
    """`right` and the bins of the case through the fp64 restatement, computed once (the fixtures hold no record of
    them: err_ref is the restatement's distance from the stored extended numbers)."""
    return F.bins_run(which, False)


def check_bins(dev, which, xpre, x, ts, block, M):
    """Behind slice ts (from 1), where the stored extended restatement holds them: `right` and the bin the slice wrote,
    the rows F.bin_rows(M) of both spins, under the rule."""
    if ts not in F.BIN_SLICES:
        return 0
    i, rows = F.BIN_SLICES.index(ts), F.bin_rows(M)
    r64 = bins64(which)
    check("slice %d right" % ts, dev.get(L.F_THERMAL_RIGHT)[0][:, rows], r64['right'][i], F.joined(x, xpre + 'right')[i])
    check("slice %d bin" % ts, dev.get(L.F_THERMAL_STACK)[0, block][:, rows], r64['bin'][i], F.joined(x, xpre + 'bin')[i])
    return 1


def test_ueg_at_123_slice_by_slice():
    """Case a8 of thermal_ueg123.npz: the recorded fields of the reference's walker through
    afq_thermal_propagate_continuous: xbar, cmf, cfb, M0 (the determinants) and the weight after every slice, G at the
    slices the fixture holds, the clip count, the final energies and nav; `right` and the bin behind the slices
    F.BIN_SLICES against the restatements (what thermal_cslice_far_kernel writes)."""
    d, x = F.golden(F.UEG), F.stored_ext()
    pre = F.UEG_A
    c = W.case_of_fixture(d, pre)
    ss, M = int(d[pre + 'stack_size']), c.M
    assert M == 123
    stored = {int(n): i for i, n in enumerate(d[pre + 'G_slices'])}
    dev = c.device(1, ss, options=FAR)
    try:
        dev.launch_trace(True)
        check("trial M0", dev.get(L.F_THERMAL_M0)[0], d[pre + 'M00'], F.joined(x, pre + 'M00'), relative=True)
        nbins_seen = 0
        for ts in range(c.L):
            used = dev.thermal_propagate_continuous(d[pre + 'xi'][ts][None], fetch_fields=True)
            numpy.testing.assert_array_equal(used[0], d[pre + 'xi'][ts])
            tag = "slice %d " % (ts + 1)
            check(tag + "xbar", dev.get(L.F_XBAR)[0], d[pre + 'xbar'][ts], F.joined(x, pre + 'xbar')[ts])
            check(tag + "cmf", dev.get(L.F_CMF)[0], d[pre + 'cmf'][ts], F.joined(x, pre + 'cmf')[ts])
            check(tag + "cfb", dev.get(L.F_CFB)[0], d[pre + 'cfb'][ts], F.joined(x, pre + 'cfb')[ts])
            check(tag + "M0", dev.get(L.F_THERMAL_M0)[0], d[pre + 'M0'][ts], F.joined(x, pre + 'M0')[ts], relative=True)
            check(tag + "weight", dev.get(L.F_WEIGHT)[0], d[pre + 'weight'][ts], F.joined(x, pre + 'weight')[ts], relative=True)
            if ts + 1 in stored:
                i = stored[ts + 1]
                check(tag + "G", dev.get(L.F_THERMAL_G)[0], d[pre + 'G'][i], F.joined(x, pre + 'G')[i])
            nbins_seen += check_bins(dev, 'ueg', pre, x, ts + 1, ts // ss, M)
        assert len(stored) >= 1 and nbins_seen == len(F.BIN_SLICES)
        assert int(dev.counters()[0]) == int(d[pre + 'nclip']) == 0
        E, nav = dev.thermal_energy()
        scale = float(numpy.max(numpy.abs(c.ops.H1diag))) * M + float(numpy.sum(c.ops.vqvec)) / c.system.vol * M
        check("energy", E[0], d[pre + 'energy'].real, F.joined(x, pre + 'energy').real, factor=scale)
        check("nav", nav[0], complex(d[pre + 'nav']).real, F.joined(x, pre + 'nav').real, factor=M)
        assert traced(dev) & (FAR_KERNELS | OTHERS) == {"thermal_cgreens_far_kernel", "thermal_cslice_far_kernel"}
    finally:
        dev.close()


def test_hubbard_8x16_slice_by_slice():
    """Case a10 of thermal_hubbard_cont_far.npz: M = 128, the bound itself, W at pitch 129; `right` and the bin behind
    the slices F.BIN_SLICES against the restatements (what thermal_cslice_dense_far_kernel writes)."""
    d, x = F.golden(F.HUBBARD), F.stored_ext()
    pre, a = 'h%d_' % F.HUBBARD_A, 'a%d_' % F.HUBBARD_A
    M = int(d[a + 'nx']) * int(d[a + 'ny'])
    assert M == 128 == far_max()
    dev = F.hubbard_device(d, a, 1, FAR)
    try:
        dev.launch_trace(True)
        check("trial M0", dev.get(L.F_THERMAL_M0)[0], d[a + 'M00'], F.joined(x, pre + 'M00'), relative=True)
        nbins_seen = 0
        for ts in range(10):
            dev.thermal_propagate_continuous(d[a + 'xi'][ts][None])
            tag = "slice %d " % (ts + 1)
            check(tag + "xbar", dev.get(L.F_XBAR)[0], d[a + 'xbar'][ts], F.joined(x, pre + 'xbar')[ts])
            check(tag + "cmf", dev.get(L.F_CMF)[0], d[a + 'cmf'][ts], F.joined(x, pre + 'cmf')[ts])
            check(tag + "cfb", dev.get(L.F_CFB)[0], d[a + 'cfb'][ts], F.joined(x, pre + 'cfb')[ts])
            check(tag + "M0", dev.get(L.F_THERMAL_M0)[0], d[a + 'M0'][ts], F.joined(x, pre + 'M0')[ts], relative=True)
            check(tag + "weight", dev.get(L.F_WEIGHT)[0], d[a + 'weight'][ts], F.joined(x, pre + 'weight')[ts], relative=True)
            nbins_seen += check_bins(dev, 'hubbard', pre, x, ts + 1, ts // int(d[a + 'stack_size']), M)
        assert nbins_seen == len(F.BIN_SLICES)
        check("last G", dev.get(L.F_THERMAL_G)[0], d[a + 'G_last'], F.joined(x, pre + 'G_last'))
        assert int(dev.counters()[0]) == int(d[a + 'nclip'])
        E, nav = dev.thermal_energy()
        H1 = numpy.asarray(W.hubbard_system(d, a).H1)
        scale = float(numpy.max(numpy.sum(numpy.abs(H1[0]), axis=0))) + float(d[a + 'U']) * M
        check("energy", E[0], d[a + 'energy'].real, F.joined(x, pre + 'energy').real, factor=scale)
        check("nav", nav[0], complex(d[a + 'nav']).real, F.joined(x, pre + 'nav').real, factor=M)
        assert traced(dev) & (FAR_KERNELS | OTHERS) == {"thermal_cgreens_far_kernel", "thermal_cslice_dense_far_kernel"}
    finally:
        dev.close()


def test_ueg_driver_at_123():
    """ThermalAFQMC with walkers: {stack_size: 5, far_basis: True} over two paths from the recorded seed: the
    reference's comb parents exactly, its estimator rows and its weights after every slice under the rule against the
    stored extended restatement of the run; a clone carries G, the bins, right and M0 of its parent bit for bit."""
    from tests.test_gpu_thermal_ueg import b_options, run_driver
    d, x = F.golden(F.UEG), F.stored_ext()
    pre, options = b_options(d, F.UEG_B)
    options['walkers']['far_basis'] = True
    rows, header, weights, parents, states, _ = run_driver(options, record_state=True)
    assert header == list(d[pre + 'header'])
    numpy.testing.assert_array_equal(numpy.array(parents), d[pre + 'parent_ix'])
    numpy.testing.assert_array_equal(numpy.array(parents), x[pre + 'parents'])
    gold = d[pre + 'blocks'].real
    assert rows.shape == gold.shape == (3, 12)
    check("rows", rows[:, 1:11], gold[:, 1:11], F.joined(x, pre + 'rx'))
    check("weights", weights, d[pre + 'weights'], F.joined(x, pre + 'wx'), relative=True)
    assert clones_are_bit_for_bit(parents, states) > 0


def test_hubbard_driver_on_10x10():
    """ThermalAFQMC with hubbard_stratonovich: 'continuous' and walkers: {far_basis: True} on 10 x 10 with 4 walkers:
    parents and the clip count exactly, rows and weights under the rule."""
    from tests.test_gpu_thermal_hubbard_cont import run_driver
    d, x = F.golden(F.HUBBARD), F.stored_ext()
    pre, xp = 'b%d_' % F.HUBBARD_B, 'hb%d_' % F.HUBBARD_B
    options = W.hubbard_driver_options(d, pre, far_basis=True)
    rows, header, weights, parents, nclip, kind = run_driver(options)
    assert kind == 'Continuous' and header == list(d[pre + 'header'])
    numpy.testing.assert_array_equal(numpy.array(parents), d[pre + 'parent_ix'])
    numpy.testing.assert_array_equal(numpy.array(parents), x[xp + 'parents'])
    assert nclip == int(d[pre + 'nclip'])
    gold = d[pre + 'blocks'].real
    cols = [0, 1, 2, 3, 4, 5, 6, 9]                    # (EHybrid is 0 and Overlap 1 in every row)
    check("rows", rows[:, 1:11][:, cols], gold[:, 1:11][:, cols], F.joined(x, xp + 'rx')[:, cols], relative=True)
    ref_w = d[pre + 'weights']
    alive = ref_w > 0
    check("weights", weights[alive], ref_w[alive], F.joined(x, xp + 'wx')[alive], relative=True)
    assert numpy.all(weights[~alive] == 0)


# ---- 3: refusals and housekeeping
def test_129_is_refused_with_the_numbers_through_the_c_abi():
    """Both continuous entry points, called as tests/test_gpu_thermal_hubbard_cont.py calls them: AFQ_EUNSUPPORTED, M,
    the 128 columns and the bound; 128 sites pass the same call."""
    from tests.test_gpu_thermal_hubbard_cont import bare_handle, configure_raw
    assert far_max() == 128
    dev, M, K = bare_handle('hubbard129')
    try:
        assert M == 129
        rc, text = configure_raw(dev, 'hubbard_continuous', M, K, options=FAR)
        assert rc == L.AFQ_EUNSUPPORTED, (rc, text)
        assert "M = 129 sites" in text and "128 columns" in text and "M <= 128" in text and "far_basis" in text
    finally:
        dev.close()
    dev, M, K = bare_handle('hubbard128')
    try:
        rc, text = configure_raw(dev, 'hubbard_continuous', M, K, options=FAR)
        assert rc == L.AFQ_OK, (rc, text)
    finally:
        dev.close()
    from tests.thermal_ueg_cases import Case
    c = Case(5.0, 2)
    assert c.M > 128
    text = refused(lambda: c.device(1, 5, options=FAR))
    assert "M = %d plane waves" % c.M in text and "128 columns" in text and "M <= 128" in text and "far_basis" in text


def test_refusals_of_the_bit():
    """The real walkers refuse the bit by name; the bit beside WIDE or STREAMED_GREENS is AFQ_EINVAL on both continuous
    entry points, in the words of the existing pair; that pair keeps its own words with the bit beside it."""
    from tests.thermal_cases import Case as HCase
    text = refused(lambda: HCase(2, 2, 4.0, 0.05).device(2, 10, 5, 5, options=FAR), L.AFQ_EINVAL)
    assert "afq_thermal_configure: far_basis belongs to the continuous fields" in text and "unknown" not in text
    for fn, me in ((lambda o: C.Chain(9).device(2, 1, o), "afq_thermal_configure_hubbard_continuous: "),
                   (lambda o: W.ueg_case(7).device(1, 5, options=o), "afq_thermal_configure_continuous: ")):
        text = refused(lambda: fn(FAR | WIDE), L.AFQ_EINVAL)
        assert text.endswith(me + "far_basis and wide_basis are two placements of the same matrices: ask for one"), text
        text = refused(lambda: fn(FAR | STREAMED), L.AFQ_EINVAL)
        assert text.endswith(me + "far_basis and streamed_greens are two placements of the same matrices: ask for one"), text
        text = refused(lambda: fn(FAR | WIDE | STREAMED), L.AFQ_EINVAL)
        assert text.endswith(me + "wide_basis and streamed_greens are two placements of the same matrices: ask for one"), text


def whole_path(dev, xis):
    out = []
    for xi in xis:
        dev.thermal_propagate_continuous(xi)
        out.append([dev.get(f) for f in STATE])
    out.append(list(dev.thermal_energy()))
    return out


def test_allocations_stand_still_and_two_runs_give_the_same_bits():
    """A whole path at M = 70 (2 bins, 2 walkers), a reset with M0 put back and the path again: the same bits, and no
    device block allocated behind the configure call (the scratch, W included, is the configure call's)."""
    ch = C.Chain(70)
    xis = numpy.random.RandomState(9).normal(size=(4, 2, 70))
    dev = ch.device(2, 2, FAR)
    try:
        n0 = dev.thermal_device_allocations()
        M00 = dev.get(L.F_THERMAL_M0)
        first = whole_path(dev, xis)
        dev.thermal_greens(1)
        dev.thermal_reset()
        dev.set(L.F_THERMAL_M0, M00)
        assert dev.thermal_state() == (0, 0, 0, 2)
        second = whole_path(dev, xis)
        assert dev.thermal_device_allocations() == n0
        for x, y in zip(first, second):
            for u, v in zip(x, y):
                numpy.testing.assert_array_equal(u, v)
    finally:
        dev.close()


def test_comb_copy_and_pack_of_a_far_population():
    """The comb clones G, the bins, right and M0 of its parents bit for bit; afq_walkers_copy and pack / unpack carry
    the same four and the weight; ONE_RDM runs on the handle."""
    from tests.test_gpu_pair_branch import DeviceBuffer
    fields = (L.F_THERMAL_G, L.F_THERMAL_STACK, L.F_THERMAL_RIGHT, L.F_THERMAL_M0, L.F_WEIGHT)
    ch = C.Chain(70)
    dev = ch.device(2, 4, FAR)
    try:
        dev.thermal_propagate_continuous(numpy.random.RandomState(2).normal(size=(4, 70)))
        dev.set(L.F_WEIGHT, numpy.array([2.2, 1e-3, 0.9, 0.9]))
        before = [dev.get(f) for f in fields[:4]]
        pix, total = dev.popcontrol_comb(0.37, 4)
        assert list(pix) == [2, 0, 1, 1] and abs(total - 4.001) < 1e-12       # teeth (k + 0.37) 4.001 / 4
        want = [b.copy() for b in before]
        for cl, kl in zip(numpy.where(pix > 1)[0], numpy.where(pix == 0)[0]):
            for x, b in zip(want, before):
                x[kl] = b[cl]
        for x, f in zip(want, fields[:4]):
            numpy.testing.assert_array_equal(dev.get(f), x)
        dev.thermal_propagate_continuous(numpy.random.RandomState(3).normal(size=(4, 70)))
        state = [dev.get(f) for f in fields]
        dev.copy_walker(2, 3)
        buf = DeviceBuffer(dev, dev.pack_bytes())
        dev.pack(0, buf.ptr.value)
        dev.unpack(1, buf.ptr.value)
        dev.sync()
        buf.free()
        for x, f in zip(state, fields):
            got = dev.get(f)
            numpy.testing.assert_array_equal(got[3], x[2])
            numpy.testing.assert_array_equal(got[1], x[0])
            numpy.testing.assert_array_equal(got[[0, 2]], x[[0, 2]])
        dev.thermal_greens(dev.thermal_state()[0])
        E, nav = dev.thermal_energy()
        res = dev.thermal_estimates(one_rdm=True)
        numpy.testing.assert_array_equal(res['cols'], numpy.concatenate([E, nav[:, None]], axis=1))
        terms = dev.get(L.F_WEIGHT)[:, None, None, None] * dev.get(L.F_THERMAL_G).real
        bound = 4 * 2.0 ** -52 * numpy.sum(numpy.abs(terms), axis=0)
        assert numpy.all(numpy.abs(res['one_rdm'] - numpy.sum(terms, axis=0)) <= bound)
    finally:
        dev.close()


def test_two_rdm_on_a_far_ueg_handle():
    """afq_thermal_estimates with ONE_RDM and TWO_RDM at M = 19 on uploaded bins, as the wide handle's test."""
    nw, nbins, ss, M = 3, 2, 2, 19
    c = W.ueg_case(M)
    stack = c.random_stack(nw, nbins, ss, 5)
    dev = c.device(nw, ss, options=FAR, L=nbins * ss)
    try:
        dev.set(L.F_THERMAL_STACK, stack)
        weights = numpy.array([0.7, 0.0, 1.3])
        dev.set(L.F_WEIGHT, weights)
        dev.thermal_greens(0)
        E, nav = dev.thermal_energy()
        res = dev.thermal_estimates(one_rdm=True, two_rdm=True)
        numpy.testing.assert_array_equal(res['cols'], numpy.concatenate([E, nav[:, None]], axis=1))
        G = dev.get(L.F_THERMAL_G)
        P = numpy.eye(M)[None, None] - numpy.swapaxes(G, -1, -2)
        _, two = dev.ueg_pair_sums(P)
        terms = weights[:, None, None, None] * two.real
        bound = nw * 2.0 ** -52 * numpy.sum(numpy.abs(terms), axis=0)
        assert numpy.all(numpy.abs(res['two_rdm'] - numpy.sum(terms, axis=0)) <= bound)
        assert numpy.max(numpy.abs(res['two_rdm'])) > 0
    finally:
        dev.close()


def test_a_run_without_the_key_launches_what_it_launched():
    """M = 19 without a bit launches the resident kernels, with WIDE the wide ones: none of the far kernels."""
    c = W.ueg_case(19)
    for options, want in ((0, {"thermal_cgreens_kernel", "thermal_cslice_kernel"}),
                          (WIDE, {"thermal_cgreens_wide_kernel", "thermal_cslice_wide_kernel"})):
        dev = c.device(1, 5, options=options)
        try:
            dev.launch_trace(True)
            dev.thermal_propagate_continuous(numpy.random.RandomState(1).normal(size=(1, c.K)))
            assert traced(dev) & (FAR_KERNELS | OTHERS) == want
        finally:
            dev.close()
