"""afq_thermal_estimates on the device: the averaged sweep, the weighted RDM sums and the route through ThermalAFQMC.

  bits      the sweep's per-bin (E, T, V, nav), the G and det it leaves and the sums are, bit for bit, the loop
            afq_thermal_greens(ts stack_size) + afq_thermal_energy on every engine (real; complex with a diagonal and
            with a dense trial; streamed), chunked or not; its launches do not depend on the number of bins.
  accuracy  per bin G, E, T, V, nav under the project's rule against the extended restatement on the stacks read back
            from the device: within 100 max(err_ref, 1e-15), err_ref the fp64 restatement's own distance from it (the
            energies' and nav's amplification factors are those of the walkers' own tests).
  sums      one_rdm and two_rdm against numpy's sums of the device's own per-walker values: per element
            nw 2^-52 sum_w |weight_w x_w| (every one of the nw products and nw adds rounds once, relative 2^-53, on a
            partial sum no larger than sum_w |weight_w x_w|, in the device's sum and in numpy's alike).
  driver    ThermalAFQMC on the cases of tests/golden/thermal_obs.npz against the reference's numerators, Nav, Weight
            and RDM blocks, within 100 max(err_ref, 1e-15) on each array's scale, err_ref the reference's distance from
            the fp64 restatement replaying the same path (tests/thermal_obs_ref.py): neither is the code under test.
Every comparison prints its figures; THERMAL_OBS_PRECISION_OUT=<file> writes the table of profiles/thermal_observables_precision.md."""
import ctypes
import os
import types

import numpy
import pytest

from pauxy_amd import _lib as L
from tests import thermal_obs_ref as R
from tests import thermal_ref as tr
from tests import thermal_ref_ext as te
from tests import thermal_ueg_ref as ur
from tests import thermal_ueg_ref_ext as ue
from tests.thermal_cases import Case as HubbardCase
from tests.thermal_hubbard_cont_cases import Chain
from tests.thermal_ueg_cases import ECUT_OF_M, Case as UegCase

pytestmark = pytest.mark.gpu

_MEASURED, _GROUP = [], [""]


@pytest.fixture(autouse=True)
def _group(request):
    _GROUP[0] = request.node.name
    yield


@pytest.fixture(scope="module", autouse=True)
def precision_table():
    yield
    out = os.environ.get("THERMAL_OBS_PRECISION_OUT")
    if not out or not _MEASURED:
        return
    lines = ["# Thermal observables: measured fraction of the accuracy bound", "",
             "Written by `THERMAL_OBS_PRECISION_OUT=<this file> pytest tests/test_gpu_thermal_obs.py` on an MI355X.  The rule:",
             "bound = 100 x max(err_ref, 1e-15) on the scale max(1, max |quantity|).  Kernel level (`sweep ...`): the device",
             "against the `numpy.clongdouble` restatement on the stacks read back from it, err_ref the fp64 restatement's",
             "distance from the extended one.  Driver level (`driver ...`): the device against the reference's fixture,",
             "err_ref the reference's distance from the fp64 restatement replaying the same path.  fraction = device / bound;",
             "per test and quantity the worst comparison is given.  The rule was not changed after these measurements.", "",
             "| test | comparison | err_ref | device | bound | fraction |", "|---|---|---|---|---|---|"]
    worst = {}
    for group, label, err_ref, err_dev, bnd in _MEASURED:
        key = (group, label.split(" @")[0])
        if key not in worst or err_dev / bnd > worst[key][2] / worst[key][3]:
            worst[key] = (label, err_ref, err_dev, bnd)
    for (group, _), (label, err_ref, err_dev, bnd) in worst.items():
        lines.append("| %s | %s | %.2e | %.2e | %.2e | %.3f |" % (group, label, err_ref, err_dev, bnd, err_dev / bnd))
    lines += ["", "Largest fraction over every comparison of the module: %.3f." % max(e / b for _, _, _, e, b in _MEASURED), ""]
    with open(out, "w") as f:
        f.write("\n".join(lines))


def check(label, got, want64, want_ext, factor=1.0):
    """device within factor x bound(err_ref) of the extended result on the scale max(1, max |quantity|)."""
    scale = max(1.0, float(numpy.max(numpy.abs(ue.ext(want_ext)))))
    err_ref, err_dev = ue.gerr(want64, want_ext, scale), ue.gerr(got, want_ext, scale)
    bnd = factor * ue.bound(err_ref)
    print("%s: err_ref %.3e device %.3e bound %.3e fraction %.3f" % (label, err_ref, err_dev, bnd, err_dev / bnd))
    _MEASURED.append((_GROUP[0], label, err_ref, err_dev, bnd))
    assert numpy.all(numpy.isfinite(numpy.asarray(got, dtype=complex))), label
    assert err_dev <= bnd, (label, err_ref, err_dev, bnd)


# ---- the four engines on uploaded stacks
_UEG, _CHAIN = {}, {}


def ueg_case(M):
    if M not in _UEG:
        _UEG[M] = UegCase(ECUT_OF_M[M], 2 if M > 7 else 1)
    return _UEG[M]


def complex_stack(M, nw, nbins, stack_size, seed):
    """thermal_ueg_cases.Case.random_stack for any M: complex bins of graded scales."""
    return UegCase.random_stack(types.SimpleNamespace(M=M, dt=0.05), nw, nbins, stack_size, seed)


class Engine(object):
    """One walker kind on a random stack: the device, and the restatement's Green's function and energy in a kit."""

    def __init__(self, name, M, nw, nbins, stack_size=2, seed=5):
        self.name, self.M, self.nw, self.nbins, self.ss = name, M, nw, nbins, stack_size
        Lts = nbins * stack_size
        streamed = L.THERMAL_STREAMED_GREENS if name.endswith('streamed') else 0
        self.ueg = name.startswith('diag')
        if name == 'real':
            nx = {4: (2, 2), 9: (3, 3), 16: (4, 4)}[M]
            c = self.case = HubbardCase(nx[0], nx[1], 4.0, 0.05)
            self.stack = c.random_stack(nw, nbins, stack_size, seed)
            self.dev = c.device(nw, Lts, stack_size, stack_size)
            self.g64, self.gx = tr.strat_greens, te.strat_greens
            self.e64 = lambda G: tr.energy(G, c.H1, c.U)
            self.ex = lambda G: tr.energy(G, c.H1, c.U, te.KitExt.dtype)
            self.e_factor, self.gbytes = c.h1_scale(), 8
        elif self.ueg:
            c = self.case = ueg_case(M)
            self.stack = c.random_stack(nw, nbins, stack_size, seed)
            self.dev = c.device(nw, stack_size, streamed, L=Lts)
            self.g64, self.gx = ur.strat_greens, ue.strat_greens
            self.e64 = lambda G: ur.energy(c.ops, G)
            self.ex = lambda G: ur.energy(c.ops_ext, G)
            self.e_factor = float(numpy.max(numpy.abs(c.ops.H1diag))) * M + float(numpy.sum(c.ops.vqvec)) / c.system.vol * M
            self.gbytes = 16
        else:
            if (M, Lts) not in _CHAIN:
                _CHAIN[M, Lts] = Chain(M, L=Lts)
            c = self.case = _CHAIN[M, Lts]
            self.stack = complex_stack(M, nw, nbins, stack_size, seed)
            self.dev = c.device(stack_size, nw, streamed)
            H1, U = numpy.asarray(c.system.H1), c.system.U
            self.g64, self.gx = ur.strat_greens, ue.strat_greens
            self.e64 = lambda G: tr.energy(G, H1, U, numpy.complex128)
            self.ex = lambda G: tr.energy(G, H1, U, ue.KitExt.dtype)
            self.e_factor = float(numpy.max(numpy.sum(numpy.abs(H1[0]), axis=0))) + U * M
            self.gbytes = 16
        self.streamed = bool(streamed)
        self.complex = name != 'real'
        try:
            self.dev.set(L.F_THERMAL_STACK, self.stack)
            rng = numpy.random.RandomState(seed + 1)
            self.weights = rng.uniform(0.2, 1.5, nw) * numpy.where(numpy.arange(nw) == 1, 0.0, 1.0)   # (one dead walker)
            self.dev.set(L.F_WEIGHT, self.weights)
        except Exception:
            self.dev.close()
            raise

    def bin_bytes(self):
        """The sweep's scratch per bin, as include/afqmc_hip.h states it."""
        mm = self.M * self.M
        return 2 * mm * self.nw * (self.gbytes + 16) + (64 * mm * self.nw if self.streamed else 0)

    def loop(self):
        """The parent's only way to the numbers: per bin afq_thermal_greens + afq_thermal_energy ->
        (per_bin [nbins, nw, 4], G [nbins, nw, 2, M, M], det of the last or None)."""
        rows, Gs = [], []
        for ts in range(self.nbins):
            self.dev.thermal_greens(ts * self.ss)
            E, nav = self.dev.thermal_energy()
            rows.append(numpy.concatenate([E, nav[:, None]], axis=1))
            Gs.append(self.dev.get(L.F_THERMAL_G))
        det = self.dev.get(L.F_THERMAL_DET) if self.complex else None
        return numpy.array(rows), numpy.array(Gs), det

    def restated(self, kit_g, kit_e, ts):
        order = ur.chain_order(ts * self.ss, self.ss, self.nbins)
        bins = [self.stack[:, b].reshape(self.nw * 2, self.M, self.M) for b in order]
        G = kit_g(bins).reshape(self.nw, 2, self.M, self.M)
        E, nav = kit_e(G)
        return G, numpy.concatenate([numpy.asarray(E), numpy.asarray(nav)[:, None]], axis=1)


def ordered_sum(per_bin):
    s = numpy.zeros_like(per_bin[0])
    for b in per_bin:
        s = s + b
    return s


ENGINES = [('real', M) for M in (4, 9, 16)] + [(e, M) for e in ('diag', 'diag_streamed') for M in (7, 19, 33)] + \
          [(e, M) for e in ('dense', 'dense_streamed') for M in (4, 9, 16)]


@pytest.mark.parametrize("name,M", ENGINES)
def test_sweep_is_the_loop_bit_for_bit(name, M):
    """nbins 1, 2, 5, 10 and 1 and 3 walkers: per_bin_out, the G (and det) left behind and cols_out against the loop;
    without AVERAGE_GF cols_out against afq_thermal_greens(slice) + afq_thermal_energy.  At 5 bins and 3 walkers also
    the accuracy of every bin's G and (E, T, V, nav) against the extended restatement."""
    for nbins in (1, 2, 5, 10):
        for nw in (1, 3):
            e = Engine(name, M, nw, nbins)
            dev = e.dev
            try:
                rows, Gs, det = e.loop()
                dev.thermal_greens(0)                       # (the sweep must not depend on what G holds)
                res = dev.thermal_estimates(average_gf=True, per_bin=True)
                numpy.testing.assert_array_equal(res['per_bin'], rows)
                numpy.testing.assert_array_equal(res['cols'], ordered_sum(rows))
                numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_G), Gs[-1])
                if det is not None:
                    numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_DET), det)
                dev.thermal_greens(dev.thermal_state()[0])
                E, nav = dev.thermal_energy()
                G0 = dev.get(L.F_THERMAL_G)
                dev.thermal_greens((nbins - 1) * e.ss)
                one = dev.thermal_estimates(per_bin=True)
                numpy.testing.assert_array_equal(one['cols'], numpy.concatenate([E, nav[:, None]], axis=1))
                numpy.testing.assert_array_equal(one['per_bin'][0], one['cols'])
                numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_G), G0)
                if nbins == 5 and nw == 3:
                    for ts in range(nbins):
                        G64, r64 = e.restated(e.g64, e.e64, ts)
                        Gx, rx = e.restated(e.gx, e.ex, ts)
                        tag = " @%s M=%d ts=%d" % (name, M, ts)
                        check("sweep G" + tag, Gs[ts], G64, Gx)
                        check("sweep E, T, V" + tag, res['per_bin'][ts][:, :3], r64[:, :3].real, rx[:, :3].real, factor=e.e_factor)
                        check("sweep nav" + tag, res['per_bin'][ts][:, 3], r64[:, 3].real, rx[:, 3].real, factor=M)
            finally:
                dev.close()


def launches(dev, fn):
    dev.launch_trace(True)
    try:
        out = fn()
        return out, {k: v[0] for k, v in dev.launch_trace_get().items()}
    finally:
        dev.launch_trace(False)


def sweep_launches(name, chunks, ueg):
    greens = {'real': 'thermal_greens_sweep_kernel', 'diag': 'thermal_cgreens_sweep_kernel', 'dense': 'thermal_cgreens_sweep_kernel',
              'diag_streamed': 'thermal_cgreens_streamed_sweep_kernel', 'dense_streamed': 'thermal_cgreens_streamed_sweep_kernel'}[name]
    want = {greens: chunks, 'thermal_rdm_kernel' if name == 'real' else 'thermal_crdm_kernel': chunks,
            'thermal_sweep_reduce_kernel': 1, 'thermal_one_rdm_kernel': 1}
    if ueg:
        want.update({'ueg_pair_kernel<0>': chunks, 'ueg_pair_finish_kernel': chunks, 'ueg_sf_wsum_kernel': 1})
    else:
        want['hubbard_energy_full_g_kernel'] = chunks
    return want


@pytest.mark.parametrize("name,M", [('real', 9), ('diag', 19), ('diag_streamed', 19), ('dense', 9), ('dense_streamed', 9)])
def test_chunked_sweep_gives_the_same_bits_and_the_launches_are_pinned(name, M):
    """5 bins under a budget of one and of two bins per chunk (a ragged last chunk) against the sweep in one chunk; the
    launch list of one chunk at 2 and at 10 bins (equal: no launch per bin), and of the chunked runs."""
    ueg = name.startswith('diag')
    kw = dict(average_gf=True, one_rdm=True, two_rdm=ueg, per_bin=True)
    e = Engine(name, M, 3, 5)
    try:
        whole, seen = launches(e.dev, lambda: e.dev.thermal_estimates(**kw))
        assert seen == sweep_launches(name, 1, ueg)
        Gw = e.dev.get(L.F_THERMAL_G)
        for per_chunk, chunks in ((1, 5), (2, 3)):
            e.dev.thermal_set_sweep_budget(per_chunk * e.bin_bytes())
            e.dev.thermal_greens(0)
            part, seen = launches(e.dev, lambda: e.dev.thermal_estimates(**kw))
            assert seen == sweep_launches(name, chunks, ueg)
            for k in whole:
                numpy.testing.assert_array_equal(part[k], whole[k])
            numpy.testing.assert_array_equal(e.dev.get(L.F_THERMAL_G), Gw)
        e.dev.thermal_set_sweep_budget(1)                   # less than a bin: a chunk still holds one
        part, seen = launches(e.dev, lambda: e.dev.thermal_estimates(**kw))
        assert seen == sweep_launches(name, 5, ueg)
        numpy.testing.assert_array_equal(part['per_bin'], whole['per_bin'])
        e.dev.thermal_set_sweep_budget(0)                   # the default again
        _, seen = launches(e.dev, lambda: e.dev.thermal_estimates(**kw))
        assert seen == sweep_launches(name, 1, ueg)
    finally:
        e.dev.close()
    for nbins in (2, 10):
        e = Engine(name, M, 3, nbins)
        try:
            _, seen = launches(e.dev, lambda: e.dev.thermal_estimates(**kw))
            assert seen == sweep_launches(name, 1, ueg), nbins
        finally:
            e.dev.close()


@pytest.mark.parametrize("name,M,average_gf", [('real', 9, True), ('diag', 19, True), ('diag', 7, False),
                                                ('diag_streamed', 19, True), ('dense', 9, True), ('dense', 16, False)])
def test_weighted_sums_against_the_devices_own_per_walker_values(name, M, average_gf):
    """one_rdm_out = sum_w weight_w Re G_w and two_rdm_out = sum_w weight_w Re two_rdm[P_w] of the G the call leaves,
    one walker of weight zero among them; a repeat gives the same bits."""
    ueg = name.startswith('diag')
    nw = 5
    e = Engine(name, M, nw, 5)
    dev = e.dev
    try:
        res = dev.thermal_estimates(average_gf=average_gf, one_rdm=True, two_rdm=ueg)
        G = dev.get(L.F_THERMAL_G)
        w = dev.get(L.F_WEIGHT)
        numpy.testing.assert_array_equal(w, e.weights)
        terms = w[:, None, None, None] * G.real
        bound = nw * 2.0 ** -52 * numpy.sum(numpy.abs(terms), axis=0)
        err = numpy.abs(res['one_rdm'] - numpy.sum(terms, axis=0))
        print("one_rdm: worst error / bound %.3f" % float(numpy.max(err / numpy.maximum(bound, 1e-300))))
        assert numpy.all(err <= bound)
        if ueg:
            P = numpy.eye(M)[None, None] - numpy.swapaxes(G, -1, -2)
            _, two = dev.ueg_pair_sums(P)
            terms = w[:, None, None, None] * two.real
            bound = nw * 2.0 ** -52 * numpy.sum(numpy.abs(terms), axis=0)
            err = numpy.abs(res['two_rdm'] - numpy.sum(terms, axis=0))
            print("two_rdm: worst error / bound %.3f" % float(numpy.max(err / numpy.maximum(bound, 1e-300))))
            assert numpy.all(err <= bound) and numpy.max(numpy.abs(res['two_rdm'])) > 0
        again = dev.thermal_estimates(average_gf=average_gf, one_rdm=True, two_rdm=ueg)
        for k in res:
            numpy.testing.assert_array_equal(again[k], res[k])
    finally:
        dev.close()


# ---- the driver on the fixture's cases
def run_driver(options):
    from pauxy_amd.context import release_context
    from pauxy_amd.qmc.thermal_afqmc import ThermalAFQMC
    state = numpy.random.get_state()
    afqmc = ThermalAFQMC(options=options)
    try:
        mixed = afqmc.estimators.estimators['mixed']
        update, raw = mixed.update, []

        def rec_update(*a, **k):
            update(*a, **k)
            raw.append((numpy.array(mixed.estimates), mixed.rdm_acc.copy(),
                        mixed.sf_acc.copy() if mixed.structure_factor else None))
        mixed.update = rec_update
        afqmc.walk.dev.launch_trace(True)
        afqmc.run()
        names = set(afqmc.walk.dev.launch_trace_get())
        afqmc.walk.dev.launch_trace(False)
        return dict(rows=numpy.array(mixed.blocks).real, header=list(mixed.header), raw=raw, names=mixed.names,
                    one_rdm=numpy.array(mixed.one_rdm), two_rdm=numpy.array(getattr(mixed, 'two_rdm', [])), launches=names)
    finally:
        numpy.random.set_state(state)
        release_context(afqmc.system, afqmc.trial)


@pytest.mark.parametrize("tag", list(R.MODELS))
def test_driver_against_the_references_numerators_and_rdm_blocks(tag):
    d, n = R.golden(), R.numbers(tag)
    out = run_driver(R.driver_options(tag))
    ref, mine = R.reference_sums(tag), R.replay(tag)
    ns = out['names']
    assert out['header'] == list(d[tag + '_header']) and out['rows'].shape == (3, 12)

    def held(label, got, want, restated):
        scale = max(1.0, float(numpy.max(numpy.abs(want))))
        err_ref, err_dev = R.distance(want, restated, scale), R.distance(got, want, scale)
        bnd = R.tolerance(err_ref)
        print("driver %s: err_ref %.3e device %.3e bound %.3e fraction %.3f" % (label, err_ref, err_dev, bnd, err_dev / bnd))
        _MEASURED.append((_GROUP[0], "driver " + label, err_ref, err_dev, bnd))
        assert numpy.all(numpy.isfinite(got)) and err_dev <= bnd, (label, err_ref, err_dev, bnd)
    for b in range(3):
        es, rdm, sf = out['raw'][b]
        at = " @block %d" % b
        for k, ix in (('weight', ns.weight), ('uweight', ns.uweight), ('enumer', ns.enumer), ('e1b', ns.e1b), ('e2b', ns.e2b),
                      ('nav', ns.nav)):
            held(k + at, es[ix].real, ref[b][k], mine[b][k])
        held("one_rdm sums" + at, rdm, ref[b]['one_rdm'], mine[b]['one_rdm'])
        held("one_rdm block" + at, out['one_rdm'][b], d[tag + '_one_rdm'][b].real, mine[b]['one_rdm'] / mine[b]['weight'])
        if ref[b]['two_rdm'] is not None:
            held("two_rdm sums" + at, sf, ref[b]['two_rdm'], mine[b]['two_rdm'])
            held("two_rdm block" + at, out['two_rdm'][b], d[tag + '_two_rdm'][b].real, mine[b]['two_rdm'] / mine[b]['weight'])
        else:
            assert sf is None
    rows, gold = out['rows'], d[tag + '_blocks'].real
    held("Nav column", rows[:, 10], gold[:, 10], numpy.array([m['nav'] / m['weight'] for m in mine]))
    if n['average_gf']:
        # the one deliberate deviation: EDenom accumulates the weights, so the energy columns are finite
        numpy.testing.assert_array_equal(rows[:, 4], rows[:, 2])
        # (the row is divided as a complex number, mixed.py:265, which rounds more than once: 4 ulp, not bits)
        assert numpy.max(numpy.abs(rows[:, 5] / (rows[:, 3] / rows[:, 4]) - 1)) <= 2.0 ** -50
        assert numpy.all(gold[:, 4] == 0) and not numpy.any(numpy.isfinite(gold[:, 5]))
    else:
        held("ETotal, E1Body, E2Body", rows[:, 5:8], gold[:, 5:8],
             numpy.array([[m['enumer'], m['e1b'], m['e2b']] for m in mine]) / numpy.array([m['weight'] for m in mine])[:, None])
    sweep = {'thermal_greens_sweep_kernel', 'thermal_cgreens_sweep_kernel', 'thermal_cgreens_streamed_sweep_kernel'}
    assert bool(out['launches'] & sweep) == n['average_gf']


def test_walker_view_fills_two_rdm_on_a_ueg_system():
    from pauxy_amd.context import release_context
    from pauxy_amd.qmc.thermal_afqmc import ThermalAFQMC
    from tests.ueg_sf_ref import pair_sums
    opts = R.driver_options('ud')
    state = numpy.random.get_state()
    afqmc = ThermalAFQMC(options=opts)
    try:
        w = afqmc.walk.walkers[1]
        two = numpy.zeros((2, 2, len(afqmc.system.qvecs)), dtype=complex)
        E = w.local_energy(afqmc.system, two_rdm=two)
        G = w.G
        P = numpy.array([numpy.eye(G.shape[-1]) - G[s].T for s in range(2)])
        want = pair_sums((afqmc.system.ikpq_i, afqmc.system.ikpq_kpq, afqmc.system.ipmq_i, afqmc.system.ipmq_pmq), P)
        assert numpy.max(numpy.abs(two - want)) <= 1e-13 * max(1.0, numpy.max(numpy.abs(want))) and numpy.max(numpy.abs(want)) > 0
        assert numpy.max(numpy.abs(numpy.array(E) - numpy.array(w.local_energy(afqmc.system)))) <= 1e-13
    finally:
        numpy.random.set_state(state)
        release_context(afqmc.system, afqmc.trial)


# The kernels a thermal driver run with none of the three options launches, recorded from the parent of this feature
# (UEG case ua, Hubbard cases ha and hc of the fixture, `estimates: {mixed: {}}`).
DEFAULT_LAUNCHES = {
    'ua': {'cap_kernel', 'clone_kernel', 'comb_plan_kernel', 'thermal_cfields_kernel', 'thermal_cgreens_kernel',
           'thermal_crdm_kernel', 'thermal_creset_kernel', 'thermal_cslice_kernel', 'thermal_cweight_kernel',
           'ueg_pair_finish_kernel', 'ueg_pair_kernel<0>', 'vbias_ueg_lds_kernel', 'vhs_ueg_kernel'},
    'ha': {'cap_kernel', 'clone_kernel', 'comb_plan_kernel', 'hubbard_energy_full_g_kernel', 'thermal_greens_kernel',
           'thermal_rdm_kernel', 'thermal_reset_kernel', 'thermal_slice_kernel', 'thermal_wrap_kernel'},
    'hc': {'cap_kernel', 'clone_kernel', 'comb_plan_kernel', 'hubbard_energy_full_g_kernel', 'thermal_cfields_dense_kernel',
           'thermal_cgreens_kernel', 'thermal_crdm_kernel', 'thermal_creset_kernel', 'thermal_cslice_dense_kernel',
           'thermal_cweight_mf_kernel'},
}


@pytest.mark.parametrize("tag", ['ua', 'ha', 'hc'])
def test_default_path_launches_what_the_parent_launched(tag):
    opts = R.driver_options(tag)
    opts['estimates'] = {'mixed': {'verbose': False}}
    out = run_driver(opts)
    print(sorted(out['launches']))
    assert out['launches'] == DEFAULT_LAUNCHES[tag]


# ---- refusals, each by code and word
def refused(fn, code, word):
    with pytest.raises(L.AfqError) as ei:
        fn()
    assert ei.value.code == code and word in str(ei.value), (ei.value.code, str(ei.value))


def raw_call(dev, what, cols=True, one=False, two=False):
    a = numpy.zeros(4 * dev.nw + 2 * dev.M * dev.M + 4 * max(1, getattr(dev, 'nq', 1)))
    p = a.ctypes.data_as(ctypes.c_void_p)
    dev._ck(dev.lib.afq_thermal_estimates(dev.h, what, p if cols else None, None, p if one else None, p if two else None))


def test_refusals():
    e = Engine('real', 4, 2, 2)
    try:
        refused(lambda: e.dev.thermal_estimates(two_rdm=True), L.AFQ_EUNSUPPORTED, "two_rdm is the structure factor of the UEG")
        refused(lambda: raw_call(e.dev, 8), L.AFQ_EINVAL, "unknown bits")
        refused(lambda: raw_call(e.dev, 0, cols=False), L.AFQ_EINVAL, "null output")
        refused(lambda: raw_call(e.dev, L.THERMAL_EST_ONE_RDM), L.AFQ_EINVAL, "null output")
        refused(lambda: e.dev.estimates_rdm(True), L.AFQ_EUNSUPPORTED, "thermal walkers: no mixed one_rdm / two_rdm")
        c = e.case
        refused(lambda: e.dev.thermal_configure(4, 2, 2, c.BT, c.BT_inv, c.BH1, c.auxf, L.THERMAL_AVERAGE_GF),
                L.AFQ_EUNSUPPORTED, "average_gf is not supported")
        refused(lambda: e.dev.thermal_estimates(), L.AFQ_ESTATE, "afq_thermal_configure")       # (the refusal unconfigured it)
    finally:
        e.dev.close()
    e = Engine('dense', 4, 2, 2)
    try:
        refused(lambda: e.dev.thermal_estimates(two_rdm=True), L.AFQ_EUNSUPPORTED, "two_rdm is the structure factor of the UEG")
    finally:
        e.dev.close()
    e = Engine('diag', 7, 2, 2)
    try:
        refused(lambda: raw_call(e.dev, L.THERMAL_EST_TWO_RDM), L.AFQ_EINVAL, "null output")
        c = e.case
        refused(lambda: e.dev.thermal_configure_continuous(4, 2, c.dt, c.full(c.BT), c.full(c.BT_inv), c.full(c.BH1), c.mf_shift,
                                                           1.0, L.THERMAL_AVERAGE_GF), L.AFQ_EUNSUPPORTED, "average_gf is not supported")
    finally:
        e.dev.close()
    from pauxy_amd.device import AfqDevice
    dev = AfqDevice(0)
    try:
        c = HubbardCase(2, 2, 4.0, 0.05)
        dev.set_system_hubbard(c.H1.astype(complex), c.U, c.na, c.nb)
        dev.walkers_alloc(2)
        refused(lambda: dev.thermal_estimates(), L.AFQ_ESTATE, "afq_thermal_configure")
    finally:
        dev.close()
