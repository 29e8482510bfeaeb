"""The `average_gf` sweep of afq_thermal_estimates on the wide body (thermal_wide.h), on the handles that run it: those
configured with AFQ_THERMAL_FAR (walkers: {far_basis: True}).  The sweep is thermal_strat.h's one kernel on a grid
(2 nw, bins) with the engine's own scratch for every work-group (thermal_cgreens_far_sweep_kernel).

1. The sweep's per-bin values, its sums and the G (and det) it leaves equal, bit for bit, the loop afq_thermal_greens per
   bin + afq_thermal_energy on the same handle, in one chunk and under a budget of one bin per chunk: UEG at M = 19, a
   Hubbard chain of 70 sites (a lane's second column), the 3 x 3 lattice with continuous fields.
2. The `average_gf` runs of thermal_obs.npz on complex walkers (UEG at M = 19 and 7, Hubbard 3 x 3 with continuous
   fields) repeated with far_basis, under the rule of tests/test_gpu_thermal_obs.py.
3. The launch list shows one Green's launch per stage, whatever the number of bins.

Handles configured with AFQ_THERMAL_WIDE or AFQ_THERMAL_DELAYED keep their refusal of AVERAGE_GF:
tests/test_gpu_thermal_wide.py and tests/test_gpu_thermal_delayed.py hold it to its words."""
import numpy
import pytest

from pauxy_amd import _lib as L
from tests import thermal_hubbard_cont_cases as C
from tests import thermal_obs_ref as R
from tests.test_gpu_thermal_obs import complex_stack, launches, ordered_sum, run_driver, ueg_case

pytestmark = pytest.mark.gpu

FAR = getattr(L, "THERMAL_FAR", 256)
SWEEP = "thermal_cgreens_far_sweep_kernel"
OTHER_SWEEPS = {"thermal_greens_sweep_kernel", "thermal_cgreens_sweep_kernel", "thermal_cgreens_streamed_sweep_kernel",
                "thermal_cgreens_wide_sweep_kernel", "thermal_greens_wide_sweep_kernel"}
SHAPES = [("diag", 19), ("chain", 70), ("lattice", 9)]


class FarHandle(object):
    """A far handle on a random stack of complex bins: diag = the UEG at M plane waves, chain = a Hubbard chain of M
    sites, lattice = the 3 x 3 lattice of thermal_hubbard_cont.npz (case a2), both with continuous fields."""

    def __init__(self, kind, M, nw, nbins, stack_size=2, seed=5):
        self.kind, self.M, self.nw, self.nbins, self.ss = kind, M, nw, nbins, stack_size
        self.ueg = kind == "diag"
        if self.ueg:
            c = ueg_case(M)
            self.stack = c.random_stack(nw, nbins, stack_size, seed)
            self.dev = c.device(nw, stack_size, FAR, L=nbins * stack_size)
        elif kind == "chain":
            self.stack = complex_stack(M, nw, nbins, stack_size, seed)
            self.dev = C.Chain(M, L=nbins * stack_size).device(stack_size, nw, FAR)
        else:
            d = C.golden()
            assert int(d['a2_nx']) * int(d['a2_ny']) == M == 9 and nbins * stack_size == 10
            self.stack = complex_stack(M, nw, nbins, stack_size, seed)
            self.dev = C.device('a2_', nw, stack_size=stack_size, options=FAR)
        try:
            self.dev.set(L.F_THERMAL_STACK, self.stack)
            rng = numpy.random.RandomState(seed + 1)
            self.weights = rng.uniform(0.2, 1.5, nw) * numpy.where(numpy.arange(nw) == 1, 0.0, 1.0)   # (one dead walker)
            self.dev.set(L.F_WEIGHT, self.weights)
        except Exception:
            self.dev.close()
            raise

    def bin_bytes(self):
        """The sweep's scratch per bin, as include/afqmc_hip.h states it for a far handle."""
        mm = self.M * self.M
        return 2 * mm * self.nw * (16 + 16) + 32 * self.nw * (4 * mm + self.M * (self.M | 1))

    def loop(self):
        rows, Gs = [], []
        for ts in range(self.nbins):
            self.dev.thermal_greens(ts * self.ss)
            E, nav = self.dev.thermal_energy()
            rows.append(numpy.concatenate([E, nav[:, None]], axis=1))
            Gs.append(self.dev.get(L.F_THERMAL_G))
        return numpy.array(rows), numpy.array(Gs), self.dev.get(L.F_THERMAL_DET)


def sweep_launches(chunks, ueg):
    want = {SWEEP: chunks, 'thermal_crdm_kernel': chunks, 'thermal_sweep_reduce_kernel': 1, 'thermal_one_rdm_kernel': 1}
    if ueg:
        want.update({'ueg_pair_kernel<0>': chunks, 'ueg_pair_finish_kernel': chunks, 'ueg_sf_wsum_kernel': 1})
    else:
        want['hubbard_energy_full_g_kernel'] = chunks
    return want


@pytest.mark.parametrize("kind,M", SHAPES)
def test_sweep_is_the_loop_bit_for_bit_with_and_without_chunks(kind, M):
    """5 bins of 2 slices, 3 walkers: per_bin_out, cols_out, and the G and det left behind against the loop; the same
    again under a budget of one bin per chunk (5 launches of the Green's kernel), of two (a ragged last chunk) and of
    less than a bin; the sums finite and not zero."""
    e = FarHandle(kind, M, 3, 5)
    dev = e.dev
    kw = dict(average_gf=True, one_rdm=True, two_rdm=e.ueg, per_bin=True)
    try:
        rows, Gs, det = e.loop()
        assert numpy.all(numpy.isfinite(rows)) and numpy.max(numpy.abs(rows)) > 0
        dev.thermal_greens(0)                               # (the sweep must not depend on what G holds)
        whole, seen = launches(dev, lambda: dev.thermal_estimates(**kw))
        assert seen == sweep_launches(1, e.ueg), seen
        numpy.testing.assert_array_equal(whole['per_bin'], rows)
        numpy.testing.assert_array_equal(whole['cols'], ordered_sum(rows))
        numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_G), Gs[-1])
        numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_DET), det)
        for budget, chunks in ((e.bin_bytes(), 5), (2 * e.bin_bytes(), 3), (1, 5)):
            dev.thermal_set_sweep_budget(budget)
            dev.thermal_greens(0)
            part, seen = launches(dev, lambda: dev.thermal_estimates(**kw))
            assert seen == sweep_launches(chunks, e.ueg), (budget, seen)
            for k in whole:
                numpy.testing.assert_array_equal(part[k], whole[k])
            numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_G), Gs[-1])
            numpy.testing.assert_array_equal(dev.get(L.F_THERMAL_DET), det)
        dev.thermal_set_sweep_budget(0)                     # the default again
        _, seen = launches(dev, lambda: dev.thermal_estimates(**kw))
        assert seen == sweep_launches(1, e.ueg)
        # without AVERAGE_GF: what it was
        dev.thermal_greens(dev.thermal_state()[0])
        E, nav = dev.thermal_energy()
        one = dev.thermal_estimates(per_bin=True)
        numpy.testing.assert_array_equal(one['cols'], numpy.concatenate([E, nav[:, None]], axis=1))
    finally:
        dev.close()


@pytest.mark.parametrize("nbins,stack_size,nw", [(1, 10, 1), (2, 5, 1), (10, 1, 3)])
def test_one_greens_launch_per_stage_whatever_the_number_of_bins(nbins, stack_size, nw):
    """1, 2 and 10 bins at M = 19, 1 and 3 walkers: the same launch list, and the loop's bits."""
    e = FarHandle("diag", 19, nw, nbins, stack_size)
    try:
        rows, Gs, det = e.loop()
        res, seen = launches(e.dev, lambda: e.dev.thermal_estimates(average_gf=True, one_rdm=True, two_rdm=True, per_bin=True))
        assert seen == sweep_launches(1, True), seen
        numpy.testing.assert_array_equal(res['per_bin'], rows)
        numpy.testing.assert_array_equal(res['cols'], ordered_sum(rows))
        numpy.testing.assert_array_equal(e.dev.get(L.F_THERMAL_G), Gs[-1])
    finally:
        e.dev.close()


AVERAGED = [tag for tag in R.MODELS if R.MODELS[tag][0] != 'hubbard' and R.numbers(tag)['average_gf']]


@pytest.mark.parametrize("tag", AVERAGED)
def test_average_gf_runs_of_the_fixture_with_far_basis(tag):
    """The driver runs of thermal_obs.npz that average over the Green's functions, on complex walkers, with
    walkers: {far_basis: True}: the numerators, Nav and the RDM blocks of every block within
    R.tolerance(err_ref) of the reference's, err_ref the restatement's distance from it (the rule of
    tests/test_gpu_thermal_obs.py); EDenom the weights; the far sweep kernel launched and no other."""
    d = R.golden()
    options = R.driver_options(tag)
    options['walkers']['far_basis'] = True
    out = run_driver(options)
    ref, mine = R.reference_sums(tag), R.replay(tag)
    ns = out['names']
    assert out['header'] == list(d[tag + '_header']) and out['rows'].shape == (3, 12)

    def held(label, got, want, restated):
        scale = max(1.0, float(numpy.max(numpy.abs(want))))
        err_ref, err_dev = R.distance(want, restated, scale), R.distance(got, want, scale)
        bnd = R.tolerance(err_ref)
        print("driver %s %s: err_ref %.3e device %.3e bound %.3e fraction %.3f" % (tag, label, err_ref, err_dev, bnd, err_dev / bnd))
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
    numpy.testing.assert_array_equal(rows[:, 4], rows[:, 2])         # (EDenom accumulates the weights)
    assert numpy.max(numpy.abs(rows[:, 5] / (rows[:, 3] / rows[:, 4]) - 1)) <= 2.0 ** -50
    assert SWEEP in out['launches'] and not out['launches'] & OTHER_SWEEPS
