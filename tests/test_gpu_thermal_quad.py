"""The quad route of the complex thermal walkers (AFQ_THERMAL_QUAD, walkers: {quad_basis: True}): the far route with four
columns per lane -- thermal_cgreens_quad_kernel (thermal_wide.h: the wide body with W in scratch and every vector at 256
entries) and the far slice kernels under their quad names with bv at 256 entries -- which carries the electron gas to the
shell of 251 plane waves and the Hubbard model with continuous fields to 256 sites.

1. Where the far route runs as well the quad route gives its bits: G, det, the bins, right, M0, the weights, the clip
   counts and the comb's parents compared with ==; the expected values are the far route's on the same inputs.
2. Where only the quad route runs, the Green's function alone (M = 129, 193, 256; 2 and 5 bins) lies within
   100 max(err_ref, 1e-15) of the stored numpy.clongdouble restatement, err_ref the stored distance of the fp64
   restatement from it (tests/golden/make_thermal_quad_ext.py).
3. Against the genuine reference under the same rule, err_ref the reference's own distance from the restatement: M = 147
   slice by slice and its driver, 16 x 16 slice by slice on the stored rows, the 12 x 12 driver; comb parents and clip
   counts exact, clones bit for bit.  Every comparison prints err_ref, device error, bound and fraction;
   THERMAL_QUAD_PRECISION_OUT=<file> writes them as the table of profiles/thermal_quad_precision.md.
4. Refusals.  5. Housekeeping."""
import os

import numpy
import pytest

from pauxy_amd import _lib as L
from tests import thermal_far_cases as F
from tests import thermal_hubbard_cont_cases as C
from tests import thermal_quad_cases as Q
from tests import thermal_wide_cases as W
from tests import thermal_ueg_ref_ext as ue

pytestmark = pytest.mark.gpu

QUAD = getattr(L, "THERMAL_QUAD", 512)                  # (a library without the option refuses the bit: every test fails)
FAR, WIDE, STREAMED = L.THERMAL_FAR, L.THERMAL_WIDE, L.THERMAL_STREAMED_GREENS
QUAD_KERNELS = {"thermal_cgreens_quad_kernel", "thermal_cslice_quad_kernel", "thermal_cslice_dense_quad_kernel"}
OTHERS = {"thermal_cgreens_kernel", "thermal_cgreens_streamed_kernel", "thermal_cgreens_wide_kernel", "thermal_cslice_kernel",
          "thermal_cslice_dense_kernel", "thermal_cslice_wide_kernel", "thermal_cslice_dense_wide_kernel",
          "thermal_cgreens_far_kernel", "thermal_cslice_far_kernel", "thermal_cslice_dense_far_kernel"}
STATE = (L.F_THERMAL_G, L.F_THERMAL_DET, L.F_THERMAL_STACK, L.F_THERMAL_RIGHT, L.F_THERMAL_M0, L.F_WEIGHT)

_MEASURED, _GROUP = [], [""]


def measured(label, err_ref, err_dev, factor=1.0):
    bnd = factor * ue.bound(err_ref)
    print("%s: err_ref %.3e device %.3e bound %.3e fraction %.3f" % (label, err_ref, err_dev, bnd, err_dev / bnd))
    _MEASURED.append((_GROUP[0], label, err_ref, err_dev, bnd))
    assert err_dev <= bnd, (label, err_ref, err_dev, bnd)


def check(label, got, ref, want_ext, relative=False, factor=1.0):
    """device within factor x bound(err_ref) of the extended result; err_ref from `ref` (the reference's record)."""
    assert numpy.all(numpy.isfinite(numpy.asarray(got, dtype=complex))), label
    if relative:
        err_ref, err_dev = ue.rerr(ref, want_ext), ue.rerr(got, want_ext)
    else:
        scale = max(1.0, float(numpy.max(numpy.abs(ue.ext(want_ext)))))
        err_ref, err_dev = ue.gerr(ref, want_ext, scale), ue.gerr(got, want_ext, scale)
    measured(label, err_ref, err_dev, factor)


@pytest.fixture(autouse=True)
def _group(request):
    _GROUP[0] = request.node.name
    yield


@pytest.fixture(scope="module", autouse=True)
def precision_table():
    yield
    out = os.environ.get("THERMAL_QUAD_PRECISION_OUT")
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


def quad_max():
    return int(L.load().afq_thermal_quad_max_basis())


def complex_stack(M, nw, nbins, stack_size, seed):
    from tests.test_gpu_thermal_wide import complex_stack as make
    return make(M, nw, nbins, stack_size, seed)


# ---- 1: the bits of the far route where both run
@pytest.mark.parametrize("M", [7, 19, 70, 128])
def test_quad_greens_has_the_bits_of_the_far_engine(M):
    """G and det on uploaded bins of a Hubbard chain, 2 walkers, 3 bins of 2 slices, at slice_ix 0 and 3: 7 is one ragged
    MFMA tile, 19 one full and one ragged, 70 a lane's second column, 128 both far classes full and the two new classes
    empty."""
    stack = complex_stack(M, 2, 3, 2, 5)
    got = {}
    for bit in (FAR, QUAD):
        dev = C.Chain(M, L=6).device(2, 2, bit)
        try:
            dev.launch_trace(True)
            dev.set(L.F_THERMAL_STACK, stack)
            out = []
            for s in (0, 3):
                dev.thermal_greens(s)
                out += [dev.get(L.F_THERMAL_G), dev.get(L.F_THERMAL_DET)]
            got[bit] = out
            names = traced(dev) & (QUAD_KERNELS | OTHERS)
            assert names == ({"thermal_cgreens_quad_kernel"} if bit == QUAD else {"thermal_cgreens_far_kernel"}), names
        finally:
            dev.close()
    assert numpy.all(numpy.isfinite(got[QUAD][0])) and numpy.max(numpy.abs(got[QUAD][0])) > 0
    for a, b in zip(got[QUAD], got[FAR]):
        numpy.testing.assert_array_equal(a, b)


def same_path_on_both_routes(make_device, xis, K, slice_kernel):
    from tests.test_gpu_thermal_far import path_arrays
    got = {}
    for bit in (FAR, QUAD):
        dev = make_device(bit)
        try:
            dev.launch_trace(True)
            got[bit] = path_arrays(dev, xis, K)
            if bit == QUAD:
                assert traced(dev) & (QUAD_KERNELS | OTHERS) == {"thermal_cgreens_quad_kernel", slice_kernel}
        finally:
            dev.close()
    assert got[QUAD][1] == got[FAR][1]                  # the clip counts
    assert len(got[QUAD][0]) == len(got[FAR][0])
    for a, b in zip(got[QUAD][0], got[FAR][0]):
        assert numpy.all(numpy.isfinite(numpy.asarray(a, dtype=complex)))
        numpy.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("pre,M", [('a0_', 7), ('a3_', 33)])
def test_quad_ueg_path_has_the_bits_of_the_far_route(pre, M):
    """Cases of thermal_ueg.npz beside a second walker: a0, M = 7, one bin of ten slices (the product right <- B right
    on every slice); a3, M = 33, five bins of 2 slices, nine MFMA tiles."""
    from tests.test_gpu_thermal_hubbard_cont import ueg_case
    c, ss, xis = ueg_case(pre)
    assert c.M == M
    same_path_on_both_routes(lambda bit: c.device(2, ss, bit), xis, c.K, "thermal_cslice_quad_kernel")


@pytest.mark.parametrize("lattice", ["6x6", "8x8"])
def test_quad_hubbard_path_has_the_bits_of_the_far_route(lattice):
    """6 x 6 (case a6 of thermal_hubbard_cont.npz at stack_size 2) and 8 x 8 (case a8 of thermal_hubbard_cont_wide.npz,
    stack_size 5), four slices each beside a second walker."""
    if lattice == "6x6":
        d = C.golden()
        same_path_on_both_routes(lambda bit: C.device('a6_', 2, stack_size=2, options=bit), d['a6_xi'][:4], 36,
                                 "thermal_cslice_dense_quad_kernel")
    else:
        d = W.golden(W.HUBBARD)
        same_path_on_both_routes(lambda bit: W.hubbard_device(d, 'a8_', 2, bit), d['a8_xi'][:4], 64,
                                 "thermal_cslice_dense_quad_kernel")


def test_quad_ueg_driver_at_81_has_the_bits_of_the_far_route():
    """The driver run b5 of thermal_ueg81.npz (6 walkers, two paths, a comb event that clones) with quad_basis and with
    far_basis: rows, weights after every slice, parents and the walkers' state around every comb, bit for bit; the
    reference's parents."""
    from tests.test_gpu_thermal_ueg import b_options, run_driver
    d = W.golden("thermal_ueg81.npz")
    runs = {}
    for key in ('far_basis', 'quad_basis'):
        pre, options = b_options(d, 5)
        options['walkers'][key] = True
        runs[key] = run_driver(options, record_state=True)
    quad, far = runs['quad_basis'], runs['far_basis']
    numpy.testing.assert_array_equal(numpy.array(quad[3]), d[pre + 'parent_ix'])
    assert numpy.any(numpy.array(quad[3]) > 1)
    numpy.testing.assert_array_equal(quad[0][:, :11], far[0][:, :11])           # (the last column is the wall time)
    numpy.testing.assert_array_equal(quad[2], far[2])
    numpy.testing.assert_array_equal(numpy.array(quad[3]), numpy.array(far[3]))
    for (qb, qa), (fb, fa) in zip(quad[4], far[4]):
        for a, b in zip(qb + qa, fb + fa):
            numpy.testing.assert_array_equal(a, b)


def sweep_handle(kind, bit, nw, nbins, stack_size=2, seed=5):
    """A handle on a random stack of complex bins, one walker dead: the UEG at M = 19, or the 3 x 3 lattice of
    thermal_hubbard_cont.npz (case a2) with continuous fields -> (device, is the UEG)."""
    from tests.test_gpu_thermal_obs import ueg_case
    if kind == "diag":
        c = ueg_case(19)
        stack = c.random_stack(nw, nbins, stack_size, seed)
        dev = c.device(nw, stack_size, bit, L=nbins * stack_size)
    else:
        assert nbins * stack_size == 10
        stack = complex_stack(9, nw, nbins, stack_size, seed)
        dev = C.device('a2_', nw, stack_size=stack_size, options=bit)
    try:
        dev.set(L.F_THERMAL_STACK, stack)
        rng = numpy.random.RandomState(seed + 1)
        dev.set(L.F_WEIGHT, rng.uniform(0.2, 1.5, nw) * numpy.where(numpy.arange(nw) == 1, 0.0, 1.0))
    except Exception:
        dev.close()
        raise
    return dev, kind == "diag"


def bin_bytes(M, nw):
    """The sweep's scratch per bin, as include/afqmc_hip.h states it for a far handle: a quad handle's is the same."""
    return 2 * M * M * nw * (16 + 16) + 32 * nw * (4 * M * M + M * (M | 1))


@pytest.mark.parametrize("kind,M", [("diag", 19), ("lattice", 9)])
def test_quad_sweep_has_the_bits_of_the_far_sweep(kind, M):
    """average_gf with one_rdm (and two_rdm on the UEG), 5 bins of 2 slices, 3 walkers: per_bin, cols, the RDMs and the G
    and det left behind, in one chunk and under a budget of two bins per chunk (three launches of the Green's kernel,
    the last ragged), against the far handle's in one chunk; one Green's launch per stage under the quad name."""
    from tests.test_gpu_thermal_obs import launches
    got = {}
    for bit in (FAR, QUAD):
        dev, ueg = sweep_handle(kind, bit, 3, 5)
        kw = dict(average_gf=True, one_rdm=True, two_rdm=ueg, per_bin=True)
        try:
            dev.thermal_greens(0)
            res, seen = launches(dev, lambda: dev.thermal_estimates(**kw))
            got[bit] = [res, dev.get(L.F_THERMAL_G), dev.get(L.F_THERMAL_DET)]
            name = "thermal_cgreens_quad_sweep_kernel" if bit == QUAD else "thermal_cgreens_far_sweep_kernel"
            assert seen[name] == 1 and seen['thermal_crdm_kernel'] == 1, seen
            assert not [k for k in seen if 'greens' in k and k != name], seen
            if bit == QUAD:
                dev.thermal_set_sweep_budget(2 * bin_bytes(M, 3))
                dev.thermal_greens(0)
                part, seen = launches(dev, lambda: dev.thermal_estimates(**kw))
                assert seen[name] == 3, seen
                got['chunks'] = [part, dev.get(L.F_THERMAL_G), dev.get(L.F_THERMAL_DET)]
        finally:
            dev.close()
    assert numpy.all(numpy.isfinite(got[QUAD][0]['per_bin'])) and numpy.max(numpy.abs(got[QUAD][0]['per_bin'])) > 0
    for mine in (got[QUAD], got['chunks']):
        assert sorted(mine[0]) == sorted(got[FAR][0])
        for k in got[FAR][0]:
            numpy.testing.assert_array_equal(mine[0][k], got[FAR][0][k])
        numpy.testing.assert_array_equal(mine[1], got[FAR][1])
        numpy.testing.assert_array_equal(mine[2], got[FAR][2])


def test_quad_sweep_above_128_is_the_loop_bit_for_bit():
    """A Hubbard chain of 130 sites (two columns in a lane's third class), 2 bins of 2 slices, 2 walkers: the sweep's
    per-bin values, its sums and the G and det it leaves against the loop afq_thermal_greens per bin +
    afq_thermal_energy on the same handle, in one chunk and with one bin per chunk -- every work-group of the grid
    (2 nw, bins) in its own scratch at four columns per lane; finite and not zero."""
    from tests.test_gpu_thermal_obs import launches, ordered_sum
    M, nw, nbins, ss = 130, 2, 2, 2
    dev = C.Chain(M, L=nbins * ss).device(ss, nw, QUAD)
    try:
        dev.set(L.F_THERMAL_STACK, complex_stack(M, nw, nbins, ss, 5))
        dev.set(L.F_WEIGHT, numpy.array([0.7, 1.3]))
        rows, Gs = [], []
        for ts in range(nbins):
            dev.thermal_greens(ts * ss)
            E, nav = dev.thermal_energy()
            rows.append(numpy.concatenate([E, nav[:, None]], axis=1))
            Gs.append(dev.get(L.F_THERMAL_G))
        rows, det = numpy.array(rows), dev.get(L.F_THERMAL_DET)
        assert numpy.all(numpy.isfinite(rows)) and numpy.max(numpy.abs(rows)) > 0 and numpy.all(numpy.isfinite(Gs))
        for budget, chunks in ((0, 1), (bin_bytes(M, nw), 2)):
            dev.thermal_set_sweep_budget(budget)
            dev.thermal_greens(0)                           # (the sweep must not depend on what G holds)
            res, seen = launches(dev, lambda: dev.thermal_estimates(average_gf=True, one_rdm=True, per_bin=True))
            assert seen["thermal_cgreens_quad_sweep_kernel"] == chunks, seen
            numpy.testing.assert_array_equal(res['per_bin'], rows)
            numpy.testing.assert_array_equal(res['cols'], ordered_sum(rows))
            numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_G), Gs[-1])
            numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_DET), det)
    finally:
        dev.close()


# ---- 2: the Green's function alone where only the quad route runs
@pytest.mark.parametrize("M,nbins", Q.GREENS_CASES)
def test_quad_greens_alone_against_the_extended_restatement(M, nbins):
    """One walker on uploaded bins of a Hubbard chain of M sites at slice_ix 0: the rows Q.rows_of(M) of G (a row crosses
    every column class) and det G under the rule, err_ref the stored distance of the fp64 restatement; what the rows do
    not hold is held to be finite.  129: one column in a lane's third class; 193: one in the fourth; 256: all full."""
    x = Q.stored_ext()
    key = Q.greens_key(M, nbins)
    rows = Q.rows_of(M)
    numpy.testing.assert_array_equal(x[key + 'rows'], rows)
    stack = Q.greens_stack(M, nbins)
    dev = C.Chain(M, L=nbins * Q.GREENS_STACK_SIZE).device(Q.GREENS_STACK_SIZE, 1, QUAD)
    try:
        dev.launch_trace(True)
        dev.set(L.F_THERMAL_STACK, stack)
        dev.thermal_greens(0)
        G, det = dev.get(L.F_THERMAL_G)[0], dev.get(L.F_THERMAL_DET)[0]
        assert traced(dev) & (QUAD_KERNELS | OTHERS) == {"thermal_cgreens_quad_kernel"}
    finally:
        dev.close()
    assert G.shape == (2, M, M) and numpy.all(numpy.isfinite(G)) and numpy.all(numpy.isfinite(det))
    measured("G M=%d bins=%d" % (M, nbins), float(x[key + 'G_err64']), Q.err_of(G[:, rows], Q.joined(x, key + 'G')))
    measured("det M=%d bins=%d" % (M, nbins), float(x[key + 'det_err64']), Q.err_of(det, Q.joined(x, key + 'det'), relative=True))


# ---- 3: the genuine reference where only the quad route runs
def clones_are_bit_for_bit(parents, states):
    from tests.test_gpu_thermal_far import clones_are_bit_for_bit as count
    return count(parents, states)


def test_ueg_at_147_slice_by_slice():
    """Case a9 of thermal_ueg147.npz: the recorded fields of the reference's walker through
    afq_thermal_propagate_continuous: xbar, cmf, cfb, M0 (the determinants) and the weight after every slice, G behind
    the last (on the rows the extended file holds), the clip count, the final energies and nav.  M = 147: 19 columns in a lane's third class."""
    d, x = Q.golden(Q.UEG), Q.stored_ext()
    pre = Q.UEG_A
    c = W.case_of_fixture(d, pre)
    ss, M = int(d[pre + 'stack_size']), c.M
    assert M == 147
    stored = {int(n): i for i, n in enumerate(d[pre + 'G_slices'])}
    g_rows = x[pre + 'G_rows']                          # (every second row and Q.rows_of(M): what the extended file holds)
    numpy.testing.assert_array_equal(g_rows, Q.ueg_g_rows(M))
    dev = c.device(1, ss, options=QUAD)
    try:
        dev.launch_trace(True)
        check("trial M0", dev.get(L.F_THERMAL_M0)[0], d[pre + 'M00'], Q.joined(x, pre + 'M00'), relative=True)
        for ts in range(c.L):
            used = dev.thermal_propagate_continuous(d[pre + 'xi'][ts][None], fetch_fields=True)
            numpy.testing.assert_array_equal(used[0], d[pre + 'xi'][ts])
            tag = "slice %d " % (ts + 1)
            check(tag + "xbar", dev.get(L.F_XBAR)[0], d[pre + 'xbar'][ts], Q.joined(x, pre + 'xbar')[ts])
            check(tag + "cmf", dev.get(L.F_CMF)[0], d[pre + 'cmf'][ts], Q.joined(x, pre + 'cmf')[ts])
            check(tag + "cfb", dev.get(L.F_CFB)[0], d[pre + 'cfb'][ts], Q.joined(x, pre + 'cfb')[ts])
            check(tag + "M0", dev.get(L.F_THERMAL_M0)[0], d[pre + 'M0'][ts], Q.joined(x, pre + 'M0')[ts], relative=True)
            check(tag + "weight", dev.get(L.F_WEIGHT)[0], d[pre + 'weight'][ts], Q.joined(x, pre + 'weight')[ts], relative=True)
            if ts + 1 in stored:
                i = stored[ts + 1]
                G = dev.get(L.F_THERMAL_G)[0]
                assert numpy.all(numpy.isfinite(G))
                check(tag + "G", G[:, g_rows], d[pre + 'G'][i][:, g_rows], Q.joined(x, pre + 'G')[i])
        assert list(stored) == [c.L]
        assert int(dev.counters()[0]) == int(d[pre + 'nclip']) == 0
        E, nav = dev.thermal_energy()
        scale = float(numpy.max(numpy.abs(c.ops.H1diag))) * M + float(numpy.sum(c.ops.vqvec)) / c.system.vol * M
        check("energy", E[0], d[pre + 'energy'].real, Q.joined(x, pre + 'energy').real, factor=scale)
        check("nav", nav[0], complex(d[pre + 'nav']).real, Q.joined(x, pre + 'nav').real, factor=M)
        assert traced(dev) & (QUAD_KERNELS | OTHERS) == {"thermal_cgreens_quad_kernel", "thermal_cslice_quad_kernel"}
    finally:
        dev.close()


def test_hubbard_16x16_slice_by_slice():
    """Case a11 of thermal_hubbard_cont_quad.npz: M = 256, the bound itself, W at pitch 257, all four column classes
    full; the scalars of every slice, and behind the last the stored rows of G, of both bins and of right (what
    thermal_cslice_dense_quad_kernel writes)."""
    d, x = Q.golden(Q.HUBBARD), Q.stored_ext()
    pre, a = 'h%d_' % Q.HUBBARD_A, 'a%d_' % Q.HUBBARD_A
    M = int(d[a + 'nx']) * int(d[a + 'ny'])
    rows = d[a + 'rows']
    assert M == 256 == quad_max() and list(rows) == list(Q.rows_of(M))
    dev = Q.hubbard_device(1, QUAD)
    try:
        dev.launch_trace(True)
        check("trial M0", dev.get(L.F_THERMAL_M0)[0], d[a + 'M00'], Q.joined(x, pre + 'M00'), relative=True)
        for ts in range(10):
            dev.thermal_propagate_continuous(d[a + 'xi'][ts][None])
            tag = "slice %d " % (ts + 1)
            check(tag + "xbar", dev.get(L.F_XBAR)[0], d[a + 'xbar'][ts], Q.joined(x, pre + 'xbar')[ts])
            check(tag + "cmf", dev.get(L.F_CMF)[0], d[a + 'cmf'][ts], Q.joined(x, pre + 'cmf')[ts])
            check(tag + "cfb", dev.get(L.F_CFB)[0], d[a + 'cfb'][ts], Q.joined(x, pre + 'cfb')[ts])
            check(tag + "M0", dev.get(L.F_THERMAL_M0)[0], d[a + 'M0'][ts], Q.joined(x, pre + 'M0')[ts], relative=True)
            check(tag + "weight", dev.get(L.F_WEIGHT)[0], d[a + 'weight'][ts], Q.joined(x, pre + 'weight')[ts], relative=True)
        G, stack, right = dev.get(L.F_THERMAL_G)[0], dev.get(L.F_THERMAL_STACK)[0], dev.get(L.F_THERMAL_RIGHT)[0]
        assert numpy.all(numpy.isfinite(G)) and numpy.all(numpy.isfinite(stack)) and numpy.all(numpy.isfinite(right))
        check("last G", G[:, rows], d[a + 'G_last'], Q.joined(x, pre + 'G_last'))
        check("last bins", stack[:, :, rows], d[a + 'bins_last'], Q.joined(x, pre + 'bins_last'))
        check("last right", right[:, rows], d[a + 'right_last'], Q.joined(x, pre + 'right_last'))
        assert int(dev.counters()[0]) == int(d[a + 'nclip'])
        E, nav = dev.thermal_energy()
        H1 = numpy.asarray(W.hubbard_system(d, a).H1)
        scale = float(numpy.max(numpy.sum(numpy.abs(H1[0]), axis=0))) + float(d[a + 'U']) * M
        check("energy", E[0], d[a + 'energy'].real, Q.joined(x, pre + 'energy').real, factor=scale)
        check("nav", nav[0], complex(d[a + 'nav']).real, Q.joined(x, pre + 'nav').real, factor=M)
        assert traced(dev) & (QUAD_KERNELS | OTHERS) == {"thermal_cgreens_quad_kernel", "thermal_cslice_dense_quad_kernel"}
    finally:
        dev.close()


def test_ueg_driver_at_147():
    """ThermalAFQMC with walkers: {stack_size: 5, quad_basis: True} over two paths from the recorded seed: the
    reference's comb parents exactly, its estimator rows and its weights after every slice under the rule against the
    stored extended restatement of the run; a clone carries G, the bins, right and M0 of its parent bit for bit."""
    from tests.test_gpu_thermal_ueg import b_options, run_driver
    d, x = Q.golden(Q.UEG), Q.stored_ext()
    pre, options = b_options(d, Q.UEG_B)
    options['walkers']['quad_basis'] = True
    rows, header, weights, parents, states, _ = run_driver(options, record_state=True)
    assert header == list(d[pre + 'header'])
    numpy.testing.assert_array_equal(numpy.array(parents), d[pre + 'parent_ix'])
    numpy.testing.assert_array_equal(numpy.array(parents), x[pre + 'parents'])
    gold = d[pre + 'blocks'].real
    assert rows.shape == gold.shape == (3, 12)
    check("rows", rows[:, 1:11], gold[:, 1:11], Q.joined(x, pre + 'rx'))
    check("weights", weights, d[pre + 'weights'], Q.joined(x, pre + 'wx'), relative=True)
    assert clones_are_bit_for_bit(parents, states) > 0


def test_hubbard_driver_on_12x12():
    """ThermalAFQMC with hubbard_stratonovich: 'continuous' and walkers: {quad_basis: True} on 12 x 12 with 4 walkers:
    parents and the clip count exactly, rows and weights under the rule."""
    from tests.test_gpu_thermal_hubbard_cont import run_driver
    d, x = Q.golden(Q.HUBBARD), Q.stored_ext()
    pre, xp = 'b%d_' % Q.HUBBARD_B, 'hb%d_' % Q.HUBBARD_B
    options = W.hubbard_driver_options(d, pre, quad_basis=True)
    rows, header, weights, parents, nclip, kind = run_driver(options)
    assert kind == 'Continuous' and header == list(d[pre + 'header'])
    numpy.testing.assert_array_equal(numpy.array(parents), d[pre + 'parent_ix'])
    numpy.testing.assert_array_equal(numpy.array(parents), x[xp + 'parents'])
    assert nclip == int(d[pre + 'nclip'])
    gold = d[pre + 'blocks'].real
    cols = [0, 1, 2, 3, 4, 5, 6, 9]                    # (EHybrid is 0 and Overlap 1 in every row)
    check("rows", rows[:, 1:11][:, cols], gold[:, 1:11][:, cols], Q.joined(x, xp + 'rx')[:, cols], relative=True)
    ref_w = d[pre + 'weights']
    alive = ref_w > 0
    check("weights", weights[alive], ref_w[alive], Q.joined(x, xp + 'wx')[alive], relative=True)
    assert numpy.all(weights[~alive] == 0)


# ---- 4: refusals
def test_257_is_refused_with_the_numbers_through_the_c_abi():
    """Both continuous entry points: AFQ_EUNSUPPORTED, M, the 256 columns, four per lane, and the bound; 256 sites pass
    the same call."""
    from tests.test_gpu_thermal_hubbard_cont import bare_handle, configure_raw
    assert quad_max() == 256
    dev, M, K = bare_handle('hubbard257')
    try:
        assert M == 257
        rc, text = configure_raw(dev, 'hubbard_continuous', M, K, options=QUAD)
        assert rc == L.AFQ_EUNSUPPORTED, (rc, text)
        assert text.endswith("thermal walkers with continuous fields, Hubbard (quad_basis): M = 257 sites are more than the 256 "
                             "columns of a wave, four per lane (M <= 256)"), text
    finally:
        dev.close()
    dev, M, K = bare_handle('hubbard256')
    try:
        rc, text = configure_raw(dev, 'hubbard_continuous', M, K, options=QUAD)
        assert rc == L.AFQ_OK, (rc, text)
    finally:
        dev.close()
    from tests.thermal_ueg_cases import Case
    c = Case(8.0, 2)                                    # (the shell behind 251: ecut 7.5 is still 251 plane waves)
    assert c.M == 257
    text = refused(lambda: c.device(1, 5, options=QUAD))
    assert "M = %d plane waves" % c.M in text and "256 columns of a wave, four per lane" in text
    assert "(M <= 256)" in text and "(quad_basis)" in text


def test_refusals_of_the_bit():
    """The real walkers refuse the bit by name; the bit beside FAR, WIDE or STREAMED_GREENS is AFQ_EINVAL on both
    continuous entry points, in the words of the existing pairs; those pairs keep their own words with the bit beside
    them."""
    from tests.thermal_cases import Case as HCase
    text = refused(lambda: HCase(2, 2, 4.0, 0.05).device(2, 10, 5, 5, options=QUAD), L.AFQ_EINVAL)
    assert "afq_thermal_configure: quad_basis belongs to the continuous fields" in text and "unknown" not in text
    text = refused(lambda: HCase(2, 2, 4.0, 0.05).device(2, 10, 5, 5, options=QUAD | 64), L.AFQ_EINVAL)
    assert "quad_basis belongs to the continuous fields" in text and "unknown" not in text          # named before bit 64
    for fn, me in ((lambda o: C.Chain(9).device(2, 1, o), "afq_thermal_configure_hubbard_continuous: "),
                   (lambda o: W.ueg_case(7).device(1, 5, options=o), "afq_thermal_configure_continuous: ")):
        for bit, word in ((FAR, "far_basis"), (WIDE, "wide_basis"), (STREAMED, "streamed_greens")):
            text = refused(lambda: fn(QUAD | bit), L.AFQ_EINVAL)
            assert text.endswith(me + "quad_basis and %s are two placements of the same matrices: ask for one" % word), text
        text = refused(lambda: fn(QUAD | FAR | WIDE), L.AFQ_EINVAL)
        assert text.endswith(me + "far_basis and wide_basis are two placements of the same matrices: ask for one"), text
        text = refused(lambda: fn(QUAD | FAR | STREAMED), L.AFQ_EINVAL)
        assert text.endswith(me + "far_basis and streamed_greens are two placements of the same matrices: ask for one"), text
        text = refused(lambda: fn(QUAD | WIDE | STREAMED), L.AFQ_EINVAL)
        assert text.endswith(me + "wide_basis and streamed_greens are two placements of the same matrices: ask for one"), text
        text = refused(lambda: fn(QUAD | 64), L.AFQ_EINVAL)
        assert text.endswith(me + "unknown option bits"), text


def test_the_far_route_still_refuses_129_in_its_own_words():
    from tests.test_gpu_thermal_hubbard_cont import bare_handle, configure_raw
    dev, M, K = bare_handle('hubbard129')
    try:
        rc, text = configure_raw(dev, 'hubbard_continuous', M, K, options=FAR)
        assert rc == L.AFQ_EUNSUPPORTED, (rc, text)
        assert text.endswith("thermal walkers with continuous fields, Hubbard (far_basis): M = 129 sites are more than the 128 "
                             "columns of a wave, two per lane (M <= 128)"), text
        rc, text = configure_raw(dev, 'hubbard_continuous', M, K, options=QUAD)
        assert rc == L.AFQ_OK, (rc, text)
    finally:
        dev.close()


# ---- 5: housekeeping
def whole_path(dev, xis):
    out = []
    for xi in xis:
        dev.thermal_propagate_continuous(xi)
        out.append([dev.get(f) for f in STATE])
    out.append(list(dev.thermal_energy()))
    return out


def test_allocations_stand_still_and_two_runs_give_the_same_bits():
    """A whole path at M = 130 (2 bins, 2 walkers: two columns in a lane's third class), a reset with M0 put back and
    the path again: the same bits, and no device block allocated behind the configure call."""
    ch = C.Chain(130)
    xis = numpy.random.RandomState(9).normal(size=(4, 2, 130))
    dev = ch.device(2, 2, QUAD)
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
                assert numpy.all(numpy.isfinite(numpy.asarray(u, dtype=complex)))
                numpy.testing.assert_array_equal(u, v)
    finally:
        dev.close()


def test_comb_copy_and_pack_of_a_quad_population():
    """At M = 130: the comb clones G, the bins, right and M0 of its parents bit for bit; afq_walkers_copy and pack /
    unpack carry the same four and the weight; ONE_RDM runs on the handle."""
    from tests.test_gpu_pair_branch import DeviceBuffer
    fields = (L.F_THERMAL_G, L.F_THERMAL_STACK, L.F_THERMAL_RIGHT, L.F_THERMAL_M0, L.F_WEIGHT)
    M = 130
    dev = C.Chain(M).device(2, 4, QUAD)
    try:
        dev.thermal_propagate_continuous(numpy.random.RandomState(2).normal(size=(4, M)))
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
        dev.thermal_propagate_continuous(numpy.random.RandomState(3).normal(size=(4, M)))
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


def test_two_rdm_on_a_quad_ueg_handle():
    """afq_thermal_estimates with ONE_RDM and TWO_RDM at M = 19 on uploaded bins, as the far handle's test."""
    nw, nbins, ss, M = 3, 2, 2, 19
    c = W.ueg_case(M)
    stack = c.random_stack(nw, nbins, ss, 5)
    dev = c.device(nw, ss, options=QUAD, L=nbins * ss)
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
    """M = 19 without a bit launches the resident kernels, with FAR the far ones, with QUAD the three quad kernels (the
    Hubbard slice kernel on a chain): no other thermal Green's or slice kernel in any of them."""
    c = W.ueg_case(19)
    for options, want in ((0, {"thermal_cgreens_kernel", "thermal_cslice_kernel"}),
                          (FAR, {"thermal_cgreens_far_kernel", "thermal_cslice_far_kernel"}),
                          (QUAD, {"thermal_cgreens_quad_kernel", "thermal_cslice_quad_kernel"})):
        dev = c.device(1, 5, options=options)
        try:
            dev.launch_trace(True)
            dev.thermal_propagate_continuous(numpy.random.RandomState(1).normal(size=(1, c.K)))
            assert traced(dev) & (QUAD_KERNELS | OTHERS) == want
        finally:
            dev.close()
    dev = C.Chain(9).device(2, 1, QUAD)
    try:
        dev.launch_trace(True)
        dev.thermal_propagate_continuous(numpy.random.RandomState(1).normal(size=(1, 9)))
        assert traced(dev) & (QUAD_KERNELS | OTHERS) == {"thermal_cgreens_quad_kernel", "thermal_cslice_dense_quad_kernel"}
    finally:
        dev.close()
