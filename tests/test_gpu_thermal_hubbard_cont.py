"""Thermal (finite-temperature) walkers of the Hubbard model with continuous fields on the device, against the
extended-precision restatement (tests/thermal_hubbard_cont_ref.py on numpy.clongdouble) under the project's rule for
thermal walkers: the device lies within 100 max(err_ref, 1e-15) of the extended result on the scale
max(1, max |quantity|); determinants and weights relative.  For the cases of the fixture err_ref is the REFERENCE's own
distance from the extended restatement (tests/golden/thermal_hubbard_cont.npz holds what the reference computed); for
shapes outside the fixture it is the fp64 restatement's.  Every comparison prints its three figures, and with
THERMAL_HUBBARD_CONT_PRECISION_OUT=<file> the module writes them as the table kept in
profiles/thermal_hubbard_continuous_precision.md.

Shapes: M = 4, 9 (odd: pitch = M), 16, 36 from the fixture; 1-D chains at the bounds M = 47 / 48 (resident Green's
function) and 63 / 64 (streamed); 1, 3 and 12 walkers."""
import hashlib
import os

import numpy
import pytest

from pauxy_amd import _lib as L
from tests import thermal_hubbard_cont_cases as C
from tests import thermal_ueg_ref_ext as ue

pytestmark = pytest.mark.gpu

_MEASURED, _GROUP = [], [""]
STATE = (L.F_THERMAL_G, L.F_THERMAL_STACK, L.F_THERMAL_RIGHT, L.F_THERMAL_M0, L.F_WEIGHT)


def check(label, got, ref, want_ext, relative=False, factor=1.0):
    """device within factor x bound(err_ref) of the extended result; err_ref from `ref` (the reference's record, or the
    fp64 restatement where there is none)."""
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
    out = os.environ.get("THERMAL_HUBBARD_CONT_PRECISION_OUT")
    if not out or not _MEASURED:
        return
    lines = ["# Thermal Hubbard walkers with continuous fields: measured fraction of the accuracy bound", "",
             "Written by `THERMAL_HUBBARD_CONT_PRECISION_OUT=<this file> pytest tests/test_gpu_thermal_hubbard_cont.py` on an",
             "MI355X.  The rule (tests/itcf_ref_ext.py): the device lies within bound = 100 x max(err_ref, 1e-15) of the",
             "`numpy.clongdouble` restatement on the scale max(1, max |quantity|); determinants, M0 and weights relative.",
             "For the fixture's cases err_ref is the reference's own distance from the restatement (the driver rows and",
             "per-slice weights included: their margin is this measured distance, not a number fixed in advance); for the",
             "other shapes it is the fp64 restatement's.  fraction = device error / bound.  Tests that compare after every",
             "slice are given by their worst slice per quantity.", "",
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


# ---- every single-walker case of the fixture, slice by slice
@pytest.mark.parametrize("k", range(C.NA))
def test_single_walker_slice_by_slice(k):
    """The recorded fields of the reference's walker through afq_thermal_propagate_continuous: xbar, cmf, cfb, the bin
    the slice wrote, G, M0 and the weight under the rule after every slice, err_ref being the reference's own record
    where the fixture holds one (xbar, cmf, cfb, M0, weight everywhere; G for M <= 16) and the fp64 restatement's for
    the bins; the clip count exactly; the final energies and nav.  k = 7: the clip fires and the walker is killed, and
    goes on moving with weight 0."""
    d = C.golden()
    pre = 'a%d_' % k
    r64, rx = C.ref_run(k, False), C.ref_run(k, True)
    ss = int(d[pre + 'stack_size'])
    M = int(d[pre + 'nx']) * int(d[pre + 'ny'])
    dev = C.device(pre, 1)
    try:
        check("trial G", dev.get(L.F_THERMAL_G)[0], d[pre + 'G0'], rx['G0'])
        check("trial M0", dev.get(L.F_THERMAL_M0)[0], d[pre + 'M00'], rx['M00'], relative=True)
        for ts in range(10):
            block = dev.thermal_state()[1]
            used = dev.thermal_propagate_continuous(d[pre + 'xi'][ts][None], fetch_fields=True)
            numpy.testing.assert_array_equal(used[0], d[pre + 'xi'][ts])
            assert dev.thermal_state() == (ts + 1, (ts + 1) // ss, (ts + 1) % ss, 10 // ss)
            tag = "slice %d " % (ts + 1)
            check(tag + "xbar", dev.get(L.F_XBAR)[0], d[pre + 'xbar'][ts], rx['xbar'][ts])
            check(tag + "cmf", dev.get(L.F_CMF)[0], d[pre + 'cmf'][ts], rx['cmf'][ts])
            check(tag + "cfb", dev.get(L.F_CFB)[0], d[pre + 'cfb'][ts], rx['cfb'][ts])
            check(tag + "bin", dev.get(L.F_THERMAL_STACK)[0, block], r64['bin'][ts], rx['bin'][ts])
            G = dev.get(L.F_THERMAL_G)[0]
            check(tag + "G", G, d[pre + 'G'][ts] if k in C.STORED_G else r64['G'][ts], rx['G'][ts])
            check(tag + "M0", dev.get(L.F_THERMAL_M0)[0], d[pre + 'M0'][ts], rx['M0'][ts], relative=True)
            w = dev.get(L.F_WEIGHT)[0]
            if d[pre + 'weight'][ts] > 0:
                check(tag + "weight", w, d[pre + 'weight'][ts], rx['weight'][ts], relative=True)
            else:
                assert w == 0.0 and rx['weight'][ts] == 0
        check("last G", dev.get(L.F_THERMAL_G)[0], d[pre + 'G_last'], rx['G'][-1])
        assert int(dev.counters()[0]) == int(d[pre + 'nclip']) == rx['nclip']
        E, nav = dev.thermal_energy()
        scale = float(numpy.max(numpy.sum(numpy.abs(C.system_and_trial(pre)[0].H1[0]), axis=0))) + float(d[pre + 'U']) * M
        check("energy", E[0], d[pre + 'energy'].real, rx['energy'].real, factor=scale)
        check("nav", nav[0], complex(d[pre + 'nav']).real, rx['nav'].real, factor=M)
        with pytest.raises(L.AfqError) as e:                                   # the path is complete
            dev.thermal_propagate_continuous(d[pre + 'xi'][0][None])
        assert e.value.code == L.AFQ_ESTATE
    finally:
        dev.close()


# ---- the driver
def b_options(k, **walkers):
    d = C.golden()
    pre = 'b%d_' % k
    return pre, {'qmc': {'timestep': float(d[pre + 'dt']), 'beta': float(d[pre + 'beta']),
                         'num_walkers': int(d[pre + 'nwalkers']), 'blocks': 2,
                         'pop_control_freq': int(d[pre + 'npop_control']), 'rng_seed': int(d[pre + 'seed'])},
                 'model': {'name': 'Hubbard', 'nx': int(d[pre + 'nx']), 'ny': int(d[pre + 'ny']), 'U': float(d[pre + 'U']),
                           'mu': float(d[pre + 'mu_system']), 'nup': int(d[pre + 'nelec']), 'ndown': int(d[pre + 'nelec'])},
                 'trial': {'name': 'one_body'},
                 'walkers': dict({'stack_size': int(d[pre + 'stack_size']), 'low_rank': False}, **walkers),
                 'propagator': {'hubbard_stratonovich': 'continuous'},
                 'estimates': {'mixed': {'verbose': False}}}


def run_driver(options):
    """-> (rows, header, weights after every slice before its cap, parents of every comb, clip count, propagator)."""
    from pauxy_amd.context import release_context
    from pauxy_amd.qmc.thermal_afqmc import ThermalAFQMC
    state = numpy.random.get_state()
    afqmc = ThermalAFQMC(options=options)
    try:
        walk, prop = afqmc.walk, afqmc.propagators
        clip0 = prop.nfb_trig
        weights, parents = [], []
        move, comb = prop.propagate_walkers, walk.pop_control

        def propagate_walkers(w, eshift=0):
            move(w, eshift)
            weights.append(walk.dev.get(L.F_WEIGHT))

        def pop_control(comm=None):
            comb(comm)
            parents.append(numpy.array(walk.last_parent_ix))
        prop.propagate_walkers, walk.pop_control = propagate_walkers, pop_control
        afqmc.run()
        mixed = afqmc.estimators.estimators['mixed']
        return (numpy.array(mixed.blocks).real, list(mixed.header), numpy.array(weights), parents,
                prop.nfb_trig - clip0, type(prop).__name__)
    finally:
        numpy.random.set_state(state)
        release_context(afqmc.system, afqmc.trial)


@pytest.mark.parametrize("k", range(C.NB))
def test_driver_with_continuous_fields_reproduces_the_references_rows(k):
    """ThermalAFQMC with propagator: {hubbard_stratonovich: 'continuous'} over two paths from the seed of the
    reference's run: the comb's parents and the clip count exactly; the rows and the weights after every slice under
    the rule, the margin being the reference's measured distance from the extended restatement of the same run.  (A
    driver that ignores the key runs discrete fields and fails here.)"""
    d = C.golden()
    pre, options = b_options(k)
    rows, header, weights, parents, nclip, kind = run_driver(options)
    assert kind == 'Continuous'
    rowsx, wx, parx, px = C.ref_driver(k, True)
    assert header == list(d[pre + 'header'])
    numpy.testing.assert_array_equal(numpy.array(parents), d[pre + 'parent_ix'])
    numpy.testing.assert_array_equal(numpy.array(parents), numpy.array(parx))
    assert nclip == int(d[pre + 'nclip']) == px.nclip
    gold = d[pre + 'blocks'].real
    assert rows.shape == gold.shape == (3, 12)
    cols = [0, 1, 2, 3, 4, 5, 6, 9]                    # (EHybrid is 0 and Overlap 1 in every row)
    check("rows b%d" % k, rows[:, 1:11][:, cols], gold[:, 1:11][:, cols], rowsx[:, cols], relative=True)
    # Overlap is the ratio of two sums of the same nw positive weights, each within (nw - 1) eps of the exact sum
    assert numpy.all(rows[:, 8] == 0)
    assert numpy.max(numpy.abs(rows[:, 9] - 1)) <= 2 * weights.shape[1] * numpy.finfo(float).eps
    ref_w = d[pre + 'weights']
    alive = ref_w > 0
    check("weights b%d" % k, weights[alive], ref_w[alive], wx[alive], relative=True)
    assert numpy.all(weights[~alive] == 0)


def test_driver_default_stays_discrete():
    """Without the key (and with 'discrete') the Hubbard driver builds ThermalDiscrete on real walkers."""
    from pauxy_amd.context import release_context
    from pauxy_amd.qmc.thermal_afqmc import ThermalAFQMC
    _, options = b_options(0)
    for prop in ({}, {'hubbard_stratonovich': 'discrete'}):
        afqmc = ThermalAFQMC(options=dict(options, propagator=prop))
        try:
            assert type(afqmc.propagators).__name__ == 'ThermalDiscrete'
            assert afqmc.walk.walkers[0].G.dtype == numpy.float64 and not afqmc.walk.dense
        finally:
            release_context(afqmc.system, afqmc.trial)


def test_driver_path_repeated_and_streamed_give_the_same_bits():
    """The same run twice, and once with walkers: {streamed_greens: True}: rows, weights and parents bit for bit."""
    _, options = b_options(0)
    rows, _, weights, parents, nclip, _ = run_driver(options)
    for other in (options, b_options(0, streamed_greens=True)[1]):
        rows2, _, weights2, parents2, nclip2, _ = run_driver(other)
        numpy.testing.assert_array_equal(rows[:, :11], rows2[:, :11])
        numpy.testing.assert_array_equal(weights, weights2)
        numpy.testing.assert_array_equal(numpy.array(parents), numpy.array(parents2))
        assert nclip == nclip2


def test_walker_views_of_a_complex_hubbard_population():
    """walker.G, walker.M0, walker.stack, walker.local_energy, reset, comb and cap as for the UEG; the population is
    configured by the propagator (ensure_configured(prop)), streamed_greens is legal for this kind, and a discrete
    propagator cannot move it afterwards."""
    from pauxy_amd.context import release_context
    from pauxy_amd.propagation.thermal_continuous import Continuous
    from pauxy_amd.propagation.thermal_hubbard import ThermalDiscrete
    from pauxy_amd.walkers.handler import Walkers
    d = C.golden()
    pre = 'a2_'
    system, trial = C.system_and_trial(pre)
    q = C.Qmc(float(d[pre + 'dt']), nwalkers=4)
    state = numpy.random.get_state()
    walk = Walkers(system, trial, q, walker_opts={'stack_size': 5, 'streamed_greens': True, 'continuous_fields': True})
    try:
        prop = Continuous({}, q, system, trial)
        w = walk.walkers[1]
        rx = C.ref_run(2, True)
        assert w.G.dtype == numpy.complex128 and walk.dense
        check("view trial G", w.G, d[pre + 'G0'], rx['G0'])
        check("view trial M0", w.M0, d[pre + 'M00'], rx['M00'], relative=True)
        numpy.random.seed(3)
        for ts in range(3):
            for ww in walk.walkers:
                prop.propagate_walker(system, ww, trial, 0)
            assert walk.time_slice == ts + 1
        assert prop.last_fields.shape == (4, 9) and w.stack.shape == (2, 2, 9, 9) and len(w.local_energy(system)) == 3
        walk.cap_weights(0.10)
        assert numpy.all(walk.dev.get(L.F_WEIGHT) <= 0.10 * walk.total_weight * (1 + 1e-15))
        walk.pop_control()
        assert int(numpy.sum(walk.last_parent_ix)) == 4
        M1 = walk.dev.get(L.F_THERMAL_M0)
        walk.reset(trial)
        assert walk.time_slice == 0 and numpy.all(walk.dev.get(L.F_WEIGHT) == 1.0)
        numpy.testing.assert_array_equal(walk.dev.get(L.F_THERMAL_M0), M1)
        with pytest.raises(RuntimeError, match='complex walkers'):
            ThermalDiscrete(system, trial, q).propagate_walkers(walk)
    finally:
        numpy.random.set_state(state)
        release_context(system, trial)


# ---- the bounds on M, and shapes the fixture does not hold
def path_against_restatement(chain, stack_size, nw, options, nslice, seed, tag):
    rng = numpy.random.RandomState(seed)
    p64, px = chain.path(stack_size, nw, False), chain.path(stack_size, nw, True)
    dev = chain.device(stack_size, nw, options)
    try:
        check(tag + " trial G", dev.get(L.F_THERMAL_G), p64.G, px.G)
        check(tag + " trial M0", dev.get(L.F_THERMAL_M0), p64.M0, px.M0, relative=True)
        for ts in range(nslice):
            xi = rng.normal(size=(nw, chain.M))
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
    finally:
        dev.close()


def refused(fn, code=None):
    with pytest.raises(L.AfqError) as e:
        fn()
    assert e.value.code == (L.AFQ_EUNSUPPORTED if code is None else code), e.value
    return str(e.value)


def test_resident_bound_47_runs_and_48_is_refused_with_the_numbers():
    """M = 47 (three MFMA tiles less one column, odd: pitch = M) runs; M = 48 is refused naming M, the Green's
    kernel, its bytes and the bound."""
    path_against_restatement(C.Chain(47), 2, 1, 0, 3, 11, "M=47")
    text = refused(lambda: C.Chain(48).device(2, 1))
    lds48 = 16 * (4 * 48 * 49 + 832) + 256
    assert "M = 48" in text and "thermal_cgreens_kernel" in text and str(lds48) in text and "M <= 47" in text
    assert "streamed_greens" in text


def test_streamed_bound_63_runs_and_64_is_refused_with_the_numbers():
    """With AFQ_THERMAL_STREAMED_GREENS the slice kernel binds: M = 63 runs, M = 64 is refused naming
    thermal_cslice_dense_kernel, its bytes and the bound."""
    path_against_restatement(C.Chain(63, L=2), 2, 1, L.THERMAL_STREAMED_GREENS, 2, 12, "M=63 streamed")
    text = refused(lambda: C.Chain(64, L=2).device(2, 1, L.THERMAL_STREAMED_GREENS))
    lds64 = 16 * (2 * 64 * 65 + 64) + 8 * 64 * 65
    assert "M = 64" in text and "thermal_cslice_dense_kernel" in text and str(lds64) in text and "M <= 63" in text


@pytest.mark.parametrize("nw", [1, 3, 12])
def test_populations_of_1_3_and_12_walkers(nw):
    """A 5-site chain (under one tile, odd), stack_size 2 of 4 slices: every branch of the in-bin counter."""
    path_against_restatement(C.Chain(5), 2, nw, 0, 4, 20 + nw, "nw=%d" % nw)


def test_a_dead_walker_still_draws_fields_and_moves():
    """Walker 1 of 3 starts with weight 0: its fields are used, its bins, G and M0 move as a live walker's do, and its
    weight stays 0."""
    chain = C.Chain(9)
    rng = numpy.random.RandomState(5)
    p64, px = chain.path(2, 3, False), chain.path(2, 3, True)
    dev = chain.device(2, 3)
    try:
        w = dev.get(L.F_WEIGHT)
        w[1] = 0.0
        dev.set(L.F_WEIGHT, w)
        p64.weight[1] = px.weight[1] = 0
        for ts in range(4):
            xi = rng.normal(size=(3, 9))
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
    """Walker 1: M0 huge, so that magn overflows: weight 0 and M0 kept.  Walker 2: the sign of one M0 flipped (cos =
    -1): weight 0 and M0 updated.  Walker 3: M0 not a number: weight 0 and M0 kept.  Walker 4: the bin the slice does
    not write is scaled by 1e80, so that G is of the order 1e-80 and det G_s, a product of 9 such pivots, is 0 in
    fp64: Mnew = 0, weight 0 and M0 kept.  Walker 0 untouched."""
    chain = C.Chain(9, L=4)
    dev = chain.device(2, 5)
    try:
        xi = numpy.random.RandomState(3).normal(size=(5, 9))
        M0 = dev.get(L.F_THERMAL_M0)
        huge = numpy.array([1e200 + 0j, 1e200 + 0j])
        M0[1] = huge
        M0[2, 0] = -M0[2, 0]
        M0[3, 1] = numpy.nan
        dev.set(L.F_THERMAL_M0, M0)
        stack = dev.get(L.F_THERMAL_STACK)
        stack[4, 1] *= 1e80                     # the other bin: det G_s ~ 1e-720 per spin, 0 in fp64
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


def whole_path(dev, xis):
    out = []
    for xi in xis:
        dev.thermal_propagate_continuous(xi)
        out.append([dev.get(f) for f in STATE])
    out.append(list(dev.thermal_energy()))
    return out


def same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            numpy.testing.assert_array_equal(u, v)


def test_streamed_resident_and_repeated_paths_give_the_same_bits():
    """One whole path at M = 16 with 5 bins: the resident Green's function twice (a reset and M0 put back in between)
    and the streamed one."""
    d = C.golden()
    pre = 'a4_'
    xis = numpy.random.RandomState(9).normal(size=(10, 3, 16))
    dev = C.device(pre, 3)
    try:
        M00 = dev.get(L.F_THERMAL_M0)
        first = whole_path(dev, xis)
        dev.thermal_reset()
        dev.set(L.F_THERMAL_M0, M00)
        assert dev.thermal_state() == (0, 0, 0, 5)
        same_bits(first, whole_path(dev, xis))
    finally:
        dev.close()
    dev = C.device(pre, 3, options=L.THERMAL_STREAMED_GREENS)
    try:
        same_bits(first, whole_path(dev, xis))
    finally:
        dev.close()
    assert int(d[pre + 'stack_size']) == 2


def test_reset_carries_m0_into_the_second_path():
    """afq_thermal_reset leaves M0 at the last path's determinants, as the reference's Walkers.reset does: the second
    path of the restatement (which the CPU tests hold to the reference's second path) is reproduced under the rule."""
    chain = C.Chain(9, L=4)
    rng = numpy.random.RandomState(21)
    p64, px = chain.path(2, 2, False), chain.path(2, 2, True)
    dev = chain.device(2, 2)
    try:
        for path in range(2):
            for ts in range(4):
                xi = rng.normal(size=(2, 9))
                p64.step(xi)
                px.step(xi)
                dev.thermal_propagate_continuous(xi)
                tag = "path %d slice %d " % (path + 1, ts + 1)
                check(tag + "M0", dev.get(L.F_THERMAL_M0), p64.M0, px.M0, relative=True)
                check_weights(tag + "weight", dev.get(L.F_WEIGHT), p64.weight, px.weight)
            last = dev.get(L.F_THERMAL_M0)
            dev.thermal_reset()
            p64.reset()
            px.reset()
            numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_M0), last)
            assert ue.rerr(last, px.M0) < 1e-6 and abs(last[0, 0] / px.M00[0] - 1) > 1e-3      # not the trial's
    finally:
        dev.close()


# ---- the entry point's refusals
def test_refusals_of_the_new_entry_point():
    from pauxy_amd.device import AfqDevice
    from tests.thermal_ueg_cases import Case as UCase
    chain = C.Chain(4)
    for bit, word in ((L.THERMAL_FREE_PROJECTION, "free_projection"), (L.THERMAL_LOW_RANK, "low_rank"),
                      (L.THERMAL_AVERAGE_GF, "average_gf")):
        assert word in refused(lambda: chain.device(2, 1, bit))
    assert "charge_decomposition" in refused(lambda: chain.device(2, 1, L.THERMAL_CHARGE), L.AFQ_EINVAL)
    assert "unknown option" in refused(lambda: chain.device(2, 1, 64), L.AFQ_EINVAL)
    refused(lambda: chain.device(3, 1), L.AFQ_EINVAL)                 # stack_size does not divide the slices
    c = UCase(0.5, 1)
    s = c.system
    dev = AfqDevice(0)
    try:
        dev.set_system_ueg(s.iA, s.iB, s.ikpq_i, s.ikpq_kpq, s.ipmq_i, s.ipmq_pmq, s.vqvec, s.vol,
                           numpy.array([s.H1[0].diagonal(), s.H1[1].diagonal()]), s.ecore, s.nup, s.ndown)
        dev.walkers_alloc(2)
        eye = numpy.array([numpy.eye(c.M)] * 2)
        assert "Hubbard" in refused(lambda: dev.thermal_configure_hubbard_continuous(10, 5, 0.05, eye, eye, eye,
                                                                                     numpy.zeros(c.M), 1.0))
    finally:
        dev.close()
    dev = chain.device(2, 4)
    try:
        assert "back-propagation" in refused(lambda: dev.bp_configure(4))
        assert "ITCF" in refused(lambda: dev.itcf_configure(2))
        assert "rdm" in refused(lambda: dev.estimates_rdm(True))
        assert "pair_branch" in refused(lambda: dev.popcontrol_pair_branch(numpy.full(2, 0.5), 4, 0.1, 4.0))
        assert "continuous" in refused(lambda: dev.thermal_propagate(numpy.full((4, 4), 0.5)), L.AFQ_ESTATE)
    finally:
        dev.close()


def test_two_ranks_are_refused():
    from pauxy_amd import device as devmod
    chain = C.Chain(4)
    s = chain.system
    ranks = [devmod.AfqDevice(0) for _ in range(2)]
    try:
        for dev in ranks:
            dev.set_system_hubbard(numpy.asarray(s.H1).astype(complex), s.U, s.nup, s.ndown)
            dev.walkers_alloc(2)
        devmod.comm_init_local(ranks)
        assert "one rank" in refused(lambda: ranks[0].thermal_configure_hubbard_continuous(
            chain.L, 2, chain.dt, chain.BT, chain.BT_inv, chain.BH1, chain.mf_shift, chain.mfc))
    finally:
        for dev in ranks:
            dev.close()


# ---- neighbours: the UEG path and the discrete Hubbard path give the bits they gave before this entry point existed
def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(numpy.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def continuous_path(dev, xis, K):
    """(digest, clip count) of a two-walker path on a fresh complex handle: the fixture's fields for walker 0, a stream
    of RandomState(42) for walker 1; every slice's state with xbar, cmf and cfb, the energies after the last slice, a
    reset and one more slice."""
    rng = numpy.random.RandomState(42)
    nslice = len(xis)
    out = []
    for ts in range(nslice + 1):
        if ts == nslice:
            dev.thermal_reset()
        xi = numpy.array([xis[ts % nslice], rng.normal(size=K)])
        dev.thermal_propagate_continuous(xi)
        out += [dev.get(f) for f in STATE + (L.F_XBAR, L.F_CMF, L.F_CFB)]
        if ts == nslice - 1:
            out += list(dev.thermal_energy())
    return digest(out), int(dev.counters()[0])


def ueg_case(pre):
    from tests.thermal_ueg_cases import Case as UCase
    d = numpy.load(os.path.join(C.HERE, "golden", "thermal_ueg.npz"))
    c = UCase(float(d[pre + 'ecut']), int(d[pre + 'nelec']), rs=float(d[pre + 'rs']), beta=float(d[pre + 'beta']),
              dt=float(d[pre + 'dt']), mu=float(d[pre + 'mu_system']), fb_bound=float(d[pre + 'fb_bound']))
    return c, int(d[pre + 'stack_size']), d[pre + 'xi'][:c.L]


def ueg_path_digest(pre='a2_', options=0, with_count=False):
    """Case a2 of thermal_ueg.npz (M = 19, two bins) beside a second walker: every slice's state, the energies, a reset
    and one more slice.  Case a4 (fb_bound 0.01) is the same basis with the clip firing."""
    c, ss, xis = ueg_case(pre)
    dev = c.device(2, ss, options)
    try:
        got = continuous_path(dev, xis, c.K)
        return got if with_count else got[0]
    finally:
        dev.close()


def hubbard_continuous_digest(pre, options):
    """A case of thermal_hubbard_cont.npz beside a second walker -> (digest, clip count).  a7: 3 x 3, odd pitch, the
    clip fires and the fixture's walker is killed; a0: 2 x 2."""
    d = C.golden()
    dev = C.device(pre, 2, options=options)
    try:
        return continuous_path(dev, d[pre + 'xi'], int(d[pre + 'nx']) * int(d[pre + 'ny']))
    finally:
        dev.close()


def hubbard_discrete_digest():
    """Case a1 of thermal_hubbard.npz (4 x 4, stack_size 10, nstblz 10), its first 20 slices on the reference's
    uniforms: the fields chosen, G, the bins and the weight after every slice, the energies."""
    from pauxy_amd.device import AfqDevice
    d = numpy.load(os.path.join(C.HERE, "golden", "thermal_hubbard.npz"))
    dev = AfqDevice(0)
    try:
        ne = d['a_nelec']
        dev.set_system_hubbard(d['a_T'].astype(complex), float(d['a_U']), int(ne[0]), int(ne[1]))
        dev.walkers_alloc(1)
        dev.thermal_configure(int(d['a_num_slices']), 10, int(d['a_nstblz']), d['a_dmat'], d['a_dmat_inv'], d['a_BH1'],
                              d['a_auxf'])
        out = []
        for ts in range(20):
            out.append(dev.thermal_propagate(d['a1_u'][ts][None], 0.0, fetch_fields=True))
            out += [dev.get(L.F_THERMAL_G), dev.get(L.F_THERMAL_STACK), dev.get(L.F_WEIGHT)]
        out += list(dev.thermal_energy())
        return digest(out)
    finally:
        dev.close()


# recorded by running the two functions above on an MI355X with the library of the commit before this entry point
UEG_DIGEST_BEFORE = "7d7d307737cafe2f20f82a1462e6e111dfcb1321c371cd06100a1bff3c4d09de"
HUBBARD_DIGEST_BEFORE = "89398e26f778b851dda36a6154d2cb62d84bacbe86142e6f105f84ba5e556a1f"


def test_ueg_and_discrete_hubbard_paths_keep_their_bits():
    assert hubbard_discrete_digest() == HUBBARD_DIGEST_BEFORE
    assert ueg_path_digest() == UEG_DIGEST_BEFORE
    dev = C.device('a0_', 2)                        # and with a dense handle alive
    try:
        dev.thermal_propagate_continuous(numpy.random.RandomState(1).normal(size=(2, 4)))
        assert hubbard_discrete_digest() == HUBBARD_DIGEST_BEFORE
        assert ueg_path_digest() == UEG_DIGEST_BEFORE
    finally:
        dev.close()


# ---- all three walker kinds held to what commit 11c5486 ("Finite-temperature AFQMC for the Hubbard model with
# continuous fields") computed, launched and refused: every literal below was recorded by running these functions on an
# MI355X with that commit's library.
STREAMED = L.THERMAL_STREAMED_GREENS
PATHS_11C5486 = {       # (kind, case, options) -> (digest, counters()[0] behind the path)
    ('hubbard', 'a7_', 0): ("092e4dd87a21a60a5e72f34f0c216463c70d118df6c3f39312b5f8b29cc766cd", 94),
    ('hubbard', 'a7_', STREAMED): ("092e4dd87a21a60a5e72f34f0c216463c70d118df6c3f39312b5f8b29cc766cd", 94),
    ('hubbard', 'a0_', 0): ("7ffb19a21451c49bea1e787db63a5ee43590a5583d6f8f48cdc184cbc954f7ea", 0),
    ('hubbard', 'a0_', STREAMED): ("7ffb19a21451c49bea1e787db63a5ee43590a5583d6f8f48cdc184cbc954f7ea", 0),
    ('ueg', 'a2_', 0): ("7d7d307737cafe2f20f82a1462e6e111dfcb1321c371cd06100a1bff3c4d09de", 0),
    ('ueg', 'a2_', STREAMED): ("7d7d307737cafe2f20f82a1462e6e111dfcb1321c371cd06100a1bff3c4d09de", 0),
    ('ueg', 'a4_', 0): ("abb0948439b0c8548a90df5d142961ee797e26af324af2834511699c5378c342", 18),
    ('ueg', 'a4_', STREAMED): ("abb0948439b0c8548a90df5d142961ee797e26af324af2834511699c5378c342", 18),
}


@pytest.mark.parametrize("key", sorted(PATHS_11C5486), ids=lambda k: "%s-%s%d" % k)
def test_continuous_paths_keep_their_bits_and_clip_counts(key):
    kind, pre, options = key
    got = hubbard_continuous_digest(pre, options) if kind == 'hubbard' else ueg_path_digest(pre, options, with_count=True)
    assert got == PATHS_11C5486[key]


def slice_launches(kind, options=0):
    """[(name, launches)] of the second slice of a path of the kind, in the order of the launch trace."""
    if kind == 'discrete':
        chain = C.Chain(4)
        s = chain.system
        from pauxy_amd.device import AfqDevice
        dev = AfqDevice(0)
        dev.set_system_hubbard(numpy.asarray(s.H1).astype(complex), s.U, s.nup, s.ndown)
        dev.walkers_alloc(2)
        dev.thermal_configure(chain.L, 2, 1, chain.BT, chain.BT_inv, chain.BH1, numpy.ones((2, 2)))
        move = lambda: dev.thermal_propagate(numpy.full((2, 4), 0.5))
    elif kind == 'planewave':
        c, ss, xis = ueg_case('a2_')
        dev = c.device(2, ss, options)
        move = lambda: dev.thermal_propagate_continuous(numpy.array([xis[0], xis[1]]))
    else:
        dev = C.device('a0_', 2, options=options)
        move = lambda: dev.thermal_propagate_continuous(numpy.random.RandomState(1).normal(size=(2, 4)))
    try:
        move()
        dev.launch_trace(True)
        move()
        dev.launch_trace(False)
        return [(name, n) for name, (n, _) in dev.launch_trace_get().items()]
    finally:
        dev.close()


LAUNCHES_11C5486 = {       # (kind, options) -> the names in the order of the trace, each launched once
    ('discrete', 0): ["thermal_slice_kernel", "thermal_greens_kernel", "thermal_wrap_kernel"],
    ('planewave', 0): ["thermal_crdm_kernel", "vbias_ueg_lds_kernel", "thermal_cfields_kernel", "vhs_ueg_kernel",
                       "thermal_cslice_kernel", "thermal_cgreens_kernel", "thermal_cweight_kernel"],
    ('planewave', STREAMED): ["thermal_crdm_kernel", "vbias_ueg_lds_kernel", "thermal_cfields_kernel", "vhs_ueg_kernel",
                              "thermal_cslice_kernel", "thermal_cgreens_streamed_kernel", "thermal_cweight_kernel"],
    ('hubbard_continuous', 0): ["thermal_crdm_kernel", "thermal_cfields_dense_kernel", "thermal_cslice_dense_kernel",
                                "thermal_cgreens_kernel", "thermal_cweight_mf_kernel"],
    ('hubbard_continuous', STREAMED): ["thermal_crdm_kernel", "thermal_cfields_dense_kernel", "thermal_cslice_dense_kernel",
                                       "thermal_cgreens_streamed_kernel", "thermal_cweight_mf_kernel"],
}


@pytest.mark.parametrize("key", sorted(LAUNCHES_11C5486), ids=lambda k: "%s%d" % k)
def test_a_slice_launches_the_kernels_it_launched(key):
    assert slice_launches(*key) == [(name, 1) for name in LAUNCHES_11C5486[key]]


def configure_raw(dev, entry, M, K, L_=4, ss=2, dt=0.05, options=0, fb_bound=1.0, nstblz=1, null=False, BT=None):
    """(code, last_error) of a configure entry point called with unit matrices (every refusal but the diagonal-trial
    one fires before an operand is read); null: no BT."""
    import ctypes
    eye = numpy.ascontiguousarray([numpy.eye(M)] * 2)
    bt = eye if BT is None else numpy.ascontiguousarray(BT, dtype=numpy.float64)
    mf, two = numpy.zeros(max(K, 1), dtype=complex), numpy.ones(4)        # (auxf [2, 2]; mf_const_fac (re, im))
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    b = None if null else p(bt)
    lib, h = dev.lib, dev.h
    if entry == 'discrete':
        rc = lib.afq_thermal_configure(h, L_, ss, nstblz, b, p(eye), p(eye), p(two), options)
    elif entry == 'planewave':
        rc = lib.afq_thermal_configure_continuous(h, L_, ss, dt, b, p(eye), p(eye), p(mf), fb_bound, options)
    else:
        rc = lib.afq_thermal_configure_hubbard_continuous(h, L_, ss, dt, b, p(eye), p(eye), p(mf), p(two), options)
    return rc, lib.afq_last_error(h).decode()


def bare_handle(system, nw=1):
    """system: 'hubbard<M>' (a chain), 'ueg<M>', or None for a handle without a system; nw 0: no walkers."""
    from pauxy_amd.device import AfqDevice
    from tests.thermal_ueg_cases import Case as UCase, ECUT_OF_M
    dev = AfqDevice(0)
    M = K = 4
    try:
        if system and system.startswith('hubbard'):
            s = C.Chain(int(system[7:])).system
            dev.set_system_hubbard(numpy.asarray(s.H1).astype(complex), s.U, s.nup, s.ndown)
            M, K = dev.M, dev.K
        elif system:
            s = UCase(3.0 if system == 'ueg81' else ECUT_OF_M[int(system[3:])], 1).system
            dev.set_system_ueg(s.iA, s.iB, s.ikpq_i, s.ikpq_kpq, s.ipmq_i, s.ipmq_pmq, s.vqvec, s.vol,
                               numpy.array([s.H1[0].diagonal(), s.H1[1].diagonal()]), s.ecore, s.nup, s.ndown)
            M, K = dev.M, dev.K
            assert M == int(system[3:])
        if nw and system:                   # (walkers need a system)
            dev.walkers_alloc(nw)
    except Exception:
        dev.close()
        raise
    return dev, M, K


HOME = {'discrete': 'hubbard4', 'planewave': 'ueg7', 'hubbard_continuous': 'hubbard4'}
AWAY = {'discrete': 'ueg7', 'planewave': 'hubbard4', 'hubbard_continuous': 'ueg7'}
# (entry point, what is wrong) -> (handle, walkers, arguments of configure_raw, code, last_error)
REFUSALS_11C5486 = {}


def _refusal(entry, what, code, text, system=0, nw=1, **kw):
    REFUSALS_11C5486[(entry, what)] = (HOME[entry] if system == 0 else system, nw, kw, code, text)


for _e, _me in (('discrete', "afq_thermal_configure"), ('planewave', "afq_thermal_configure_continuous"),
                ('hubbard_continuous', "afq_thermal_configure_hubbard_continuous")):
    _refusal(_e, 'null operand', L.AFQ_EINVAL, _me + ": null operand", null=True)
    _refusal(_e, 'free_projection', L.AFQ_EUNSUPPORTED,
             "thermal walkers: free_projection is not supported (constrained path only)", options=L.THERMAL_FREE_PROJECTION)
    _refusal(_e, 'low_rank', L.AFQ_EUNSUPPORTED, "thermal walkers: low_rank is not supported", options=L.THERMAL_LOW_RANK)
    _refusal(_e, 'average_gf', L.AFQ_EUNSUPPORTED, "thermal walkers: average_gf is not supported",
             options=L.THERMAL_AVERAGE_GF)
    _refusal(_e, 'unknown bits', L.AFQ_EINVAL, _me + ": unknown option bits", options=64)
    _refusal(_e, 'unknown bits beside streamed', L.AFQ_EINVAL,
             _me + (": streamed_greens belongs to the continuous fields (the real walkers fit to M = 64 as they are)"
                    if _e == 'discrete' else ": unknown option bits"), options=64 | STREAMED)
    _refusal(_e, 'every bit', L.AFQ_EUNSUPPORTED if _e == 'discrete' else L.AFQ_EINVAL,
             {'discrete': "thermal walkers: charge_decomposition is not supported (spin decomposition only)",
              'planewave': _me + ": charge_decomposition belongs to the discrete fields",
              'hubbard_continuous': _me + ": charge_decomposition belongs to the discrete fields (the continuous form is "
                                          "the charge form alone)"}[_e], options=127)
    _refusal(_e, 'no system', L.AFQ_ESTATE, _me + ": set the system and allocate the walkers first", system=None)
    _refusal(_e, 'no walkers', L.AFQ_ESTATE, _me + ": set the system and allocate the walkers first", nw=0)
    _refusal(_e, 'stack_size 3 of 4 slices', L.AFQ_EINVAL,
             _me + ": stack_size must divide ntime_slices (%s >= 1)" % ("all" if _e == 'discrete' else "both"), ss=3)
    _refusal(_e, 'stack_size 0', L.AFQ_EINVAL,
             _me + ": stack_size must divide ntime_slices (%s >= 1)" % ("all" if _e == 'discrete' else "both"), ss=0)
    _refusal(_e, 'no slices', L.AFQ_EINVAL,
             _me + ": stack_size must divide ntime_slices (%s >= 1)" % ("all" if _e == 'discrete' else "both"), L_=0)
_refusal('discrete', 'charge_decomposition', L.AFQ_EUNSUPPORTED,
         "thermal walkers: charge_decomposition is not supported (spin decomposition only)", options=L.THERMAL_CHARGE)
_refusal('planewave', 'charge_decomposition', L.AFQ_EINVAL,
         "afq_thermal_configure_continuous: charge_decomposition belongs to the discrete fields", options=L.THERMAL_CHARGE)
_refusal('hubbard_continuous', 'charge_decomposition', L.AFQ_EINVAL,
         "afq_thermal_configure_hubbard_continuous: charge_decomposition belongs to the discrete fields (the continuous "
         "form is the charge form alone)", options=L.THERMAL_CHARGE)
_refusal('discrete', 'streamed_greens', L.AFQ_EINVAL, "afq_thermal_configure: streamed_greens belongs to the continuous "
         "fields (the real walkers fit to M = 64 as they are)", options=STREAMED)
_refusal('discrete', 'nstblz 0', L.AFQ_EINVAL, "afq_thermal_configure: stack_size must divide ntime_slices (all >= 1)",
         nstblz=0)
_refusal('discrete', 'wrong system', L.AFQ_EUNSUPPORTED, "thermal walkers: Hubbard systems only (no Generic / UEG)",
         system=AWAY['discrete'])
_refusal('planewave', 'wrong system', L.AFQ_EUNSUPPORTED, "thermal walkers with continuous fields: UEG systems only (no "
         "Generic, no continuous Hubbard)", system=AWAY['planewave'])
_refusal('hubbard_continuous', 'wrong system', L.AFQ_EUNSUPPORTED, "thermal walkers with continuous fields and a dense "
         "trial: Hubbard systems only (no Generic)", system=AWAY['hubbard_continuous'])
# (a wrong system is refused before its size: the UEG's 7 plane waves on the Hubbard entry points, and streamed too)
_refusal('hubbard_continuous', 'wrong system, streamed', L.AFQ_EUNSUPPORTED, "thermal walkers with continuous fields and "
         "a dense trial: Hubbard systems only (no Generic)", system=AWAY['hubbard_continuous'], options=STREAMED)
_refusal('planewave', 'dt 0', L.AFQ_EINVAL, "afq_thermal_configure_continuous: dt must be positive, fb_bound not negative",
         dt=0.0)
_refusal('planewave', 'dt negative', L.AFQ_EINVAL,
         "afq_thermal_configure_continuous: dt must be positive, fb_bound not negative", dt=-0.05)
_refusal('planewave', 'fb_bound negative', L.AFQ_EINVAL,
         "afq_thermal_configure_continuous: dt must be positive, fb_bound not negative", fb_bound=-1.0)
_refusal('planewave', 'dt before the trial', L.AFQ_EINVAL,
         "afq_thermal_configure_continuous: dt must be positive, fb_bound not negative", dt=0.0, BT=numpy.ones((2, 7, 7)))
_refusal('planewave', 'stack_size before dt', L.AFQ_EINVAL,
         "afq_thermal_configure_continuous: stack_size must divide ntime_slices (both >= 1)", ss=3, dt=0.0)
_refusal('planewave', 'dense trial', L.AFQ_EUNSUPPORTED, "thermal walkers with continuous fields: a diagonal trial density "
         "matrix only (OneBody on plane waves)", BT=numpy.ones((2, 7, 7)))
_refusal('hubbard_continuous', 'dt 0', L.AFQ_EINVAL, "afq_thermal_configure_hubbard_continuous: dt must be positive", dt=0.0)
_refusal('hubbard_continuous', 'dt negative', L.AFQ_EINVAL, "afq_thermal_configure_hubbard_continuous: dt must be positive",
         dt=-0.05)
_refusal('hubbard_continuous', 'stack_size before dt', L.AFQ_EINVAL,
         "afq_thermal_configure_hubbard_continuous: stack_size must divide ntime_slices (both >= 1)", ss=3, dt=0.0)
# the four bounds with their numbers; the bound is refused before stack_size and dt are looked at
_refusal('hubbard_continuous', 'M = 48 resident', L.AFQ_EUNSUPPORTED,
         "thermal walkers with continuous fields, Hubbard: M = 48 sites need 164096 bytes of LDS for the "
         "complex Green's function (thermal_cgreens_kernel), a work-group has 163840 (M <= 47); "
         "AFQ_THERMAL_STREAMED_GREENS (streamed_greens) keeps T in device memory and reaches further",
         system='hubbard48', ss=3, dt=0.0)
_refusal('hubbard_continuous', 'M = 64 streamed', L.AFQ_EUNSUPPORTED,
         "thermal walkers with continuous fields, Hubbard (streamed_greens): M = 64 sites need 167424 "
         "bytes of LDS for the slice kernel (thermal_cslice_dense_kernel), a work-group has 163840 (M <= "
         "63)", system='hubbard64', options=STREAMED, ss=3)
_refusal('planewave', 'M = 57 resident', L.AFQ_EUNSUPPORTED,
         "thermal walkers with continuous fields: M = 57 plane waves need 221504 bytes of LDS for the "
         "complex Green's function, a work-group has 163840 (M <= 47); AFQ_THERMAL_STREAMED_GREENS "
         "(streamed_greens) keeps T in device memory and reaches further",
         system='ueg57', ss=3, dt=0.0)
_refusal('planewave', 'M = 81 streamed', L.AFQ_EUNSUPPORTED,
         "thermal walkers with continuous fields (streamed_greens): M = 81 plane waves need 314928 bytes "
         "of LDS for the slice kernel (thermal_cslice_kernel), a work-group has 163840 (M <= 57)",
         system='ueg81', options=STREAMED, ss=3)


@pytest.mark.parametrize("key", sorted(REFUSALS_11C5486), ids=lambda k: ("%s-%s" % k).replace(" ", "_"))
def test_every_refusal_keeps_its_code_and_its_words(key):
    system, nw, kw, code, text = REFUSALS_11C5486[key]
    dev, M, K = bare_handle(system, nw)
    try:
        assert configure_raw(dev, key[0], M, K, **kw) == (code, text)
        # and the handle holds no thermal walkers afterwards
        assert dev.lib.afq_thermal_reset(dev.h) == L.AFQ_ESTATE
    finally:
        dev.close()


# ---- the ABI
def test_abi_of_the_new_entry_points():
    """The library exports afq_thermal_configure_hubbard_continuous and afq_thermal_left_table with the table's
    signatures; a fresh bin is the host-built BT^stack_size bit for bit, and the bin after one slice at stack_size 1
    is left_0 right to the rounding of one product."""
    lib = L.load()
    for name in ("afq_thermal_configure_hubbard_continuous", "afq_thermal_left_table"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert L.SIGNATURES["afq_thermal_configure_hubbard_continuous"] == [
        L._h, L.c_int, L.c_int, L.c_double, L._dp, L._dp, L._dp, L._dp, L._dp, L.c_int]
    from pauxy_amd.propagation.thermal_continuous import left_table
    chain = C.Chain(9, L=2)
    pw, left = left_table(chain.BT, chain.BT_inv, 1)
    dev = chain.device(1, 1)
    try:
        numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_STACK)[0, 0], pw.astype(complex))      # a fresh bin
        xi = numpy.random.RandomState(2).normal(size=(1, 9))
        dev.thermal_propagate_continuous(xi)
        right = dev.get(L.F_THERMAL_RIGHT)[0]
        want = left[0] @ right
        got = dev.get(L.F_THERMAL_STACK)[0, 0]
        assert ue.gerr(got, want) <= 9 * 4 * numpy.finfo(float).eps        # one product of inner dimension 9
    finally:
        dev.close()
