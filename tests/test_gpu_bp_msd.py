"""The back-propagation window of a multi-determinant (NOMSD) trial on the device (afq_bp_update_msd, k_bp_msd.hip;
DESIGN row 8f-2).  The reference has no such window, so every case is held to the extended-precision restatement of the
specification (tests/bp_msd_ref.py) on the fields and weights read back from the device, under the rule of
tests/itcf_ref_ext.py: bound(err_ref), err_ref the fp64 restatement's own distance from the extended one.

The kernel path a case is meant to reach is named in its id and asserted from the launch trace of the window:
  fused    the backward pass loops the determinants through prop_fused_kernel over one V
  stacked  the GEMM chain (M > 104, more than 32 electrons per spin): the determinants of a walker as one
           column-stacked operand, k_bp_msd_onebody / k_bp_msd_taylor ("stacked GEMM": per-wave register engine,
           "stacked ring GEMM": the work-group ring engine, M > 128 with 64 or more walkers)
  greens   small / blocked: greens_small_kernel or k_greens_big with gj_mfma_kernel, with a per-walker trial
and in every window the HS potential is built once per step, never once per determinant."""
import os

import numpy
import pytest
import torch.multiprocessing as mp

from oracle import afqmc_ref as ref
from pauxy_amd import _lib as L, systems, trial as trial_mod
from pauxy_amd.context import release_context
from pauxy_amd.device import AfqDevice
from pauxy_amd.propagation import setup
from pauxy_amd.qmc.afqmc import AFQMC
from tests import bp_msd_ref as R, test_gpu_multirank as mr
from tests.helpers import make_device
from tests.itcf_models import generic_model

pytestmark = pytest.mark.gpu
VHS = ('k_vhs_generic', 'vhs_cplx_launch')


def has(names, sub):
    return any(sub in n for n in names)


def count(trace, subs):
    return sum(int(v[0]) for k, v in trace.items() if any(s in k for s in subs))


class Case(object):
    """A Generic system, nd determinants (the first the closed-shell real RHF one with rhf_first) and a device holding
    them as its trial with nw perturbed walkers."""

    def __init__(self, M, K, na, nb, nd, nw, hermitian=False, rhf_first=False, seed=3, dead=(), force_bias=True,
                 copies=False):
        model, s, rng = generic_model(M, K, na, nb, seed, hermitian=hermitian, rhf=rhf_first)
        ne = na + nb
        base = numpy.asarray(model.psi)
        dets = [base if (d == 0 and rhf_first) or copies else base + 0.05 * (rng.rand(M, ne) + 1j * rng.rand(M, ne))
                for d in range(nd)]
        self.dets = numpy.array(dets, dtype=complex)
        self.coeffs = numpy.array([0.8 + 0.1j, 0.4 - 0.3j, -0.25 + 0.2j, 0.3 + 0.3j][:nd])
        self.s, self.rng, self.M, self.K, self.na, self.nb, self.nw, self.nd = s, rng, M, K, na, nb, nw, nd
        self.dt = model.dt
        t = trial_mod.MultiDetTrial(s, (self.coeffs, self.dets), init=base)
        self.BH1, self.mf = setup.generic_propagator_arrays(s, t, self.dt)
        self.H1 = numpy.asarray(s.H1).astype(complex)
        dev = AfqDevice(0)
        per = M * ne
        dev.set_system_generic(s.hs_pot, t._rchol[:per], self.H1, s.ecore, na, nb)
        dev.set_trial_multi(self.dets, self.coeffs, t._rchol)
        dev.set_propagator(self.BH1, self.mf, self.dt, force_bias=force_bias)
        dev.walkers_alloc(nw)
        phi = numpy.array([base + 0.1 * (rng.rand(M, ne) + 1j * rng.rand(M, ne)) for _ in range(nw)])
        dev.set(L.F_PHI, phi)
        dev.set(L.F_OT, dev.calc_overlap())
        if len(dead):
            w = dev.get(L.F_WEIGHT).copy()
            w[list(dead)] = 0.0
            dev.set(L.F_WEIGHT, w)
        self.dev, self.trial = dev, t
        self.energy = (self.H1, s.ecore, numpy.asarray(s.hs_pot))

    def steps(self, n, eshift=0.2):
        xs = []
        for _ in range(n):
            self.dev.propagate(self.rng.normal(size=(self.nw, self.K)), eshift)
            xs.append(self.dev.get(L.F_XSHIFTED).copy())
        return xs

    def weights(self, restore, nstblz):
        """The weight of every walker in the window: F_WEIGHT, times the recorded factors read back through the
        single-determinant window's denominator of one walker at a time (tests/itcf_models.py: restore_factors)."""
        dev = self.dev
        w0 = dev.get(L.F_WEIGHT).copy()
        if restore is None:
            return w0.astype(complex)
        out = numpy.zeros(self.nw, dtype=complex)
        for i in range(self.nw):
            if w0[i] == 0:
                continue
            one = numpy.zeros(self.nw)
            one[i] = 1.0
            dev.set(L.F_WEIGHT, one)
            out[i] = w0[i] * dev.bp_update(self.dets[0], nstblz, restore, reset=False)[1]
        dev.set(L.F_WEIGHT, w0)
        return out

    def window(self, case, xs, phi0, nstblz, restore=None, energy=False, reset=True, sample=False, fused=None,
               greens=None, stacked=None, closed=None):
        dev = self.dev
        wt = self.weights(restore, nstblz)
        dev.launch_trace(True)
        before = dev.counters(n=8).copy()
        got = dev.bp_update_msd(self.dets, self.coeffs, nstblz, restore, energy, reset=reset)
        took = dev.counters(n=8) - before
        trace = dev.launch_trace_get()
        dev.launch_trace(False)
        names = set(trace)
        # (complex vectors: a real and an imaginary product per build; the backward pass walks the whole configured
        #  history, steps a walker has not recorded find no live walker)
        per_build = 2 if has(names, 'vhs_cplx_launch') else 1
        said = ['V built %d x for a history of %d steps' % (count(trace, VHS) // per_build, dev.nbp)]
        assert count(trace, VHS) == dev.nbp * per_build, trace
        if fused is not None:
            assert has(names, 'prop_fused_kernel') == fused, sorted(names)
            assert has(names, 'k_bp_msd_taylor') == (not fused), sorted(names)
            said.append('backward pass: ' + ('prop_fused_kernel per determinant' if fused else 'stacked GEMM chain'))
        if stacked is not None:
            assert has(names, 'k_bp_msd_taylor: ' + stacked) and has(names, 'k_bp_msd_onebody: ' + stacked), sorted(names)
            assert not has(names, 'k_apply_exponential') and not has(names, 'k_onebody'), sorted(names)
            said.append(stacked)
        if closed is not None:
            # afq_counters [3]: walker steps in the fused propagator's closed-shell deal -- the closed-shell determinant's
            # steps and no other determinant's
            assert int(took[3]) == closed, took
            said.append('closed-shell deal: %d walker steps' % int(took[3]))
        if greens == 'blocked':
            assert has(names, 'gj_mfma_kernel') and has(names, 'k_greens_big'), sorted(names)
            said.append('greens: blocked Gauss-Jordan')
        elif greens == 'small':
            assert has(names, 'greens_small_kernel'), sorted(names)
            said.append('greens: small')
        for k in ('bp_msd_detw_kernel', 'bp_msd_gsum_kernel', 'bp_msd_finish_kernel', 'bp_msd_accumulate_kernel'):
            assert has(names, k), (k, sorted(names))
        R.compare(case, got, numpy.asarray(self.s.hs_pot), self.BH1, self.dt, numpy.array(xs), phi0, self.dets,
                  self.coeffs, self.na, nstblz, wt, self.energy if energy else None, sample=sample, path=', '.join(said))
        return got


def run(case, M, K, na, nb, nd, nw, nbp=3, nstblz=1, restore=None, energy=False, hermitian=False, rhf_first=False,
        dead=(), sample=False, seed=3, **path):
    c = Case(M, K, na, nb, nd, nw, hermitian=hermitian, rhf_first=rhf_first, seed=seed, dead=dead)
    c.dev.bp_configure(nbp)
    phi0 = c.dev.get(L.F_PHI).copy()
    xs = c.steps(nbp)
    w = c.dev.get(L.F_WEIGHT)
    assert all(w[d] == 0 for d in dead) and numpy.isfinite(w).all() and (w > 0).sum() == nw - len(dead)
    # a dead walker records nothing: its history is incomplete, and it counts in neither numerator nor denominator
    recorded = c.dev.bp_steps()
    assert all(recorded[d] < nbp for d in dead) and all(recorded[i] == nbp for i in range(nw) if i not in dead)
    c.window(case, xs, phi0, nstblz, restore, energy, sample=sample, **path)
    c.dev.close()


SHAPES = [
    ("M=12 3+3 ndet=2 [fused]", dict(M=12, K=9, na=3, nb=3, nd=2, nw=4, nbp=4, nstblz=2, fused=True)),
    ("M=12 3+3 ndet=3 energies [fused]", dict(M=12, K=9, na=3, nb=3, nd=3, nw=4, nbp=4, nstblz=2, energy=True, fused=True)),
    ("M=24 6+5 ndet=4 nstblz=1 [fused]", dict(M=24, K=12, na=6, nb=5, nd=4, nw=5, nbp=4, nstblz=1, fused=True)),
    ("M=24 6+5 ndet=4 nstblz=2 full restore, energies [fused]", dict(M=24, K=12, na=6, nb=5, nd=4, nw=5, nbp=4, nstblz=2, restore='full', energy=True, fused=True)),
    ("M=24 6+5 ndet=4 nstblz>=nbp partial restore [fused]", dict(M=24, K=12, na=6, nb=5, nd=4, nw=5, nbp=4, nstblz=9, restore='partial', fused=True)),
    ("M=24 5+6 ndet=2 na<nb, two dead [fused]", dict(M=24, K=12, na=5, nb=6, nd=2, nw=6, nbp=3, nstblz=2, dead=(0, 4), fused=True)),
    ("M=100 25+25 ndet=3 first RHF nw=8 [fused, small]", dict(M=100, K=20, na=25, nb=25, nd=3, nw=8, nbp=3, nstblz=2, rhf_first=True, fused=True, greens='small', closed=8 * 3)),
    ("M=120 20+19 ndet=2 [stacked GEMM, small]", dict(M=120, K=12, na=20, nb=19, nd=2, nw=3, nbp=3, nstblz=2, fused=False, stacked='stacked GEMM', greens='small')),
    ("M=120 20+20 ndet=3 first RHF [stacked GEMM]", dict(M=120, K=12, na=20, nb=20, nd=3, nw=3, nbp=3, nstblz=2, rhf_first=True, fused=False, stacked='stacked GEMM')),
    ("M=128 64+64 ndet=2 [stacked GEMM, blocked Gauss-Jordan]", dict(M=128, K=12, na=64, nb=64, nd=2, nw=2, nbp=2, nstblz=1, fused=False, stacked='stacked GEMM', greens='blocked')),
    ("(H) M=64 7+5 ndet=2 energies [fused]", dict(M=64, K=12, na=7, nb=5, nd=2, nw=4, nbp=3, nstblz=2, hermitian=True, energy=True, fused=True)),
    ("(H) M=64 40+37 ndet=2 [stacked GEMM]", dict(M=64, K=12, na=40, nb=37, nd=2, nw=3, nbp=3, nstblz=2, hermitian=True, fused=False, stacked='stacked GEMM')),
    ("M=64 7+5 ndet=2 nw=33 [ring VHS, fused]", dict(M=64, K=12, na=7, nb=5, nd=2, nw=33, nbp=2, nstblz=1, fused=True)),
    ("M=64 7+5 ndet=2 nw=64 one dead [ring VHS, fused]", dict(M=64, K=12, na=7, nb=5, nd=2, nw=64, nbp=2, nstblz=1, dead=(63,), fused=True)),
    ("M=64 7+5 ndet=3 nw=65 [ring VHS, fused]", dict(M=64, K=12, na=7, nb=5, nd=3, nw=65, nbp=2, nstblz=1, fused=True)),
    ("M=132 10+9 ndet=2 nw=64 two dead [stacked ring GEMM; sampled]", dict(M=132, K=12, na=10, nb=9, nd=2, nw=64, nbp=3, nstblz=2, dead=(5, 63), sample=True, fused=False, stacked='stacked ring GEMM')),
    ("M=132 20+20 ndet=3 first RHF nw=65 [stacked ring GEMM; sampled]", dict(M=132, K=12, na=20, nb=20, nd=3, nw=65, nbp=2, nstblz=1, rhf_first=True, sample=True, fused=False, stacked='stacked ring GEMM')),
]


@pytest.mark.parametrize("case,kw", [pytest.param(c, k, id=c.replace(' ', '_')) for c, k in SHAPES])
def test_shapes_and_paths(case, kw):
    run(case, **kw)


# ---------------------------------------------------------------------------------------------------- identities
def rel(a, b):
    return float(numpy.max(numpy.abs(numpy.asarray(a) - numpy.asarray(b))) / max(1.0, float(numpy.max(numpy.abs(b)))))


def single_handle(c, det, nw):
    """A single-determinant handle with determinant `det` as its trial and the propagator arrays of case c."""
    t = trial_mod.SingleDetTrial(c.s, det)
    model = ref.RefModel('generic', c.M, c.na, c.nb, t.psi, c.BH1, c.mf, c.dt, hs_pot=c.s.hs_pot, rchol=t._rchol,
                         H1=c.H1, ecore=c.s.ecore)
    return make_device(model, nw, force_bias=False)


@pytest.mark.parametrize("shape", [(24, 12, 6, 5, 4, True), (120, 12, 20, 19, 3, False)], ids=["fused", "stacked"])
def test_two_determinants_against_the_single_determinant_path(shape):
    """G_bp S = w_1 G_1 + w_2 G_2 with G_d from afq_bp_update(phi_bp0 = D_d) on a single-determinant handle fed the same
    fields (no force bias, so that the recorded fields are the drawn ones on every handle), w_d from detw_out; and with
    nstblz >= nbp the window's S against the forward overlap of the walkers now."""
    M, K, na, nb, nw, fused = shape
    nbp = 4
    c = Case(M, K, na, nb, 2, nw, force_bias=False)
    phi0 = c.dev.get(L.F_PHI).copy()
    singles = [single_handle(c, c.dets[d], nw) for d in range(2)]
    for d in [c.dev] + singles:
        d.set(L.F_PHI, phi0)
        d.set(L.F_OT, d.calc_overlap())
        d.bp_configure(nbp)
    xi = c.rng.normal(size=(nbp, nw, K))
    for x in xi:
        for d in [c.dev] + singles:
            d.propagate(x, 0.0)
            assert numpy.array_equal(d.get(L.F_XSHIFTED), c.dev.get(L.F_XSHIFTED))
    for nstblz in (2, 9):
        E, den, G, detw = c.dev.bp_update_msd(c.dets, c.coeffs, nstblz, None, False, reset=False)
        wt = c.dev.get(L.F_WEIGHT)
        want = 0
        for w in range(nw):
            one = numpy.zeros(nw)
            one[w] = 1.0
            Gd = []
            for d in range(2):
                singles[d].set(L.F_WEIGHT, one)
                _, dd, g = singles[d].bp_update(c.dets[d], nstblz, None, reset=False)
                assert dd == 1.0
                Gd.append(g)
            want = want + wt[w] * (detw[w, 0] * Gd[0] + detw[w, 1] * Gd[1])
        assert abs(numpy.sum(detw, axis=1) - 1).max() < 1e-13
        print("BPMSD-SINGLE | %s nstblz=%d | sum_d w_d G_d vs the single-determinant windows: %.2e" % (
            'fused' if fused else 'stacked', nstblz, rel(G, want)))
        assert rel(G, want) < 1e-12 and abs(den - wt.sum()) < 1e-12 * abs(wt.sum())
    # backward and forward agree on the overlap: the normalised weights of the never re-orthogonalised window are
    # conj(c_d) <D_d|phi_n> / sum of the walkers as they are now
    c.dev.greens(want_G=False)
    fw = c.dev.det_weights()
    assert rel(detw, fw / fw.sum(axis=1)[:, None]) < 1e-11
    for d in [c.dev] + singles:
        d.close()


@pytest.mark.parametrize("shape", [(24, 12, 6, 5, 4, 2), (120, 12, 20, 19, 3, 2)], ids=["fused", "stacked"])
def test_identities_on_the_device(shape):
    """Three copies of one determinant with any c_d are the single-determinant window (afq_bp_update on the same
    handle: the init_walker path); D_d -> D_d U_d with c_d -> c_d / det U_d changes nothing."""
    M, K, na, nb, nw, nstblz = shape
    nbp = 4
    c = Case(M, K, na, nb, 3, nw, copies=True)
    c.dev.bp_configure(nbp)
    c.steps(nbp)
    E, den, G, detw = c.dev.bp_update_msd(c.dets, c.coeffs, nstblz, 'full', True, reset=False)
    E1, den1, G1 = c.dev.bp_update(c.dets[0], nstblz, 'full', True, reset=False)
    print("BPMSD-COPIES | M=%d | G %.2e E %.2e" % (M, rel(G, G1), rel(E, E1)))
    assert rel(G, G1) < 1e-12 and rel(E, E1) < 1e-12 and abs(den - den1) <= 1e-14 * abs(den1)
    assert rel(detw, numpy.tile(c.coeffs.conj() / c.coeffs.conj().sum(), (nw, 1))) < 1e-12
    c.dev.close()
    c = Case(M, K, na, nb, 3, nw)
    c.dev.bp_configure(nbp)
    c.steps(nbp)
    a = c.dev.bp_update_msd(c.dets, c.coeffs, nstblz, None, True, reset=False)
    rng = numpy.random.RandomState(2)
    dets, coeffs = c.dets.copy(), c.coeffs.copy()
    for d in range(3):
        Ua = numpy.linalg.qr(rng.normal(size=(na, na)) + 1j * rng.normal(size=(na, na)))[0]
        Ub = numpy.linalg.qr(rng.normal(size=(nb, nb)) + 1j * rng.normal(size=(nb, nb)))[0]
        dets[d] = numpy.hstack([c.dets[d][:, :na].dot(Ua), c.dets[d][:, na:].dot(Ub)])
        coeffs[d] = c.coeffs[d] / (numpy.linalg.det(Ua) * numpy.linalg.det(Ub))
    b = c.dev.bp_update_msd(dets, coeffs, nstblz, None, True, reset=False)
    print("BPMSD-ROTATED | M=%d | G %.2e E %.2e detw %.2e" % (M, rel(b[2], a[2]), rel(b[0], a[0]), rel(b[3], a[3])))
    assert rel(b[2], a[2]) < 1e-11 and rel(b[0], a[0]) < 1e-11 and rel(b[3], a[3]) < 1e-11 and b[1] == a[1]
    c.dev.close()


def test_init_walker_window_on_a_multi_determinant_handle():
    """afq_bp_update (one determinant: trial.init) on the multi-determinant handle gives what a single-determinant
    handle gives for the same fields."""
    c = Case(24, 12, 6, 5, 2, 4, force_bias=False)
    phi0 = c.dev.get(L.F_PHI).copy()
    init = numpy.asarray(c.trial.init)
    sd = single_handle(c, init, 4)
    for d in (c.dev, sd):
        d.set(L.F_PHI, phi0)
        d.set(L.F_OT, d.calc_overlap())
        d.bp_configure(3)
    for x in c.rng.normal(size=(3, 4, 12)):
        for d in (c.dev, sd):
            d.propagate(x, 0.0)
    sd.set(L.F_WEIGHT, c.dev.get(L.F_WEIGHT))
    a = c.dev.bp_update(init, 2, None, True)
    b = sd.bp_update(init, 2, None, True)
    assert rel(a[2], b[2]) < 1e-13 and rel(a[0], b[0]) < 1e-13 and a[1] == b[1]
    c.dev.propagate(c.rng.normal(size=(4, 12)), 0.0)          # the walk goes on
    assert numpy.isfinite(c.dev.get(L.F_WEIGHT)).all() and numpy.isfinite(c.dev.get(L.F_PHI)).all()
    c.dev.close()
    sd.close()


# ---------------------------------------------------------------------------------------------------- launches
def step_launches(dev, xi):
    dev.launch_trace(True)
    dev.propagate(xi, 0.1)
    trace = dev.launch_trace_get()
    dev.launch_trace(False)
    return {k: int(v[0]) for k, v in trace.items()}


def test_v_is_built_once_per_step_and_the_forward_step_is_untouched():
    """M=120, ndet=3: the launch trace of one window has nbp launches of the VHS builder (not ndet nbp) and the stacked
    products; the launch list of a forward step is the same before the window, after it, and on a handle that never
    configured back-propagation, apart from the history kernel."""
    nbp, nd, nw, K = 4, 3, 3, 12
    c = Case(120, K, 20, 19, nd, nw)
    plain = Case(120, K, 20, 19, nd, nw)
    xi = numpy.random.RandomState(1).normal(size=(nbp + 2, nw, K))
    for d in (c.dev, plain.dev):
        d.propagate(xi[0], 0.1)                              # (first step: one-off set-up launches)
    c.dev.bp_configure(nbp)
    before = step_launches(c.dev, xi[1])
    never = step_launches(plain.dev, xi[1])
    for x in xi[2:nbp + 1]:
        c.dev.propagate(x, 0.1)
        plain.dev.propagate(x, 0.1)
    c.dev.launch_trace(True)
    c.dev.bp_update_msd(c.dets, c.coeffs, 2)
    trace = {k: int(v[0]) for k, v in c.dev.launch_trace_get().items()}
    c.dev.launch_trace(False)
    assert count({k: (v,) for k, v in trace.items()}, VHS) == nbp, trace
    assert trace.get('k_bp_msd_taylor: stacked GEMM') == nbp * 6 and not has(trace, 'k_apply_exponential'), trace
    assert sum(v for k, v in trace.items() if 'k_bp_msd_onebody' in k) in (2 * nbp, 4 * nbp), trace     # (one per spin when BH1 differs)
    assert not has(trace, 'prop_fused_kernel')
    after = step_launches(c.dev, xi[nbp + 1])
    never2 = step_launches(plain.dev, xi[nbp + 1])
    assert before == after, (before, after)
    strip = lambda t: {k: v for k, v in t.items() if 'bp_push_kernel' not in k}        # noqa: E731
    assert has(before, 'bp_push_kernel') and not has(never, 'bp_push_kernel')
    assert strip(before) == never == never2, (before, never)
    assert numpy.array_equal(c.dev.get(L.F_PHI), plain.dev.get(L.F_PHI))
    c.dev.close()
    plain.dev.close()


WALK = (L.F_PHI, L.F_WEIGHT, L.F_UNSCALED_WEIGHT, L.F_OT, L.F_HYBRID_ENERGY, L.F_PHASE, L.F_DETR)


def state(dev):
    return [dev.get(f).copy() for f in WALK] + [dev.get(L.F_GHALF).copy(), dev.get(L.F_G).copy(), dev.det_weights().copy()]


@pytest.mark.parametrize("shape", [(24, 12, 6, 5, 5, False), (100, 20, 25, 25, 8, True), (120, 12, 20, 19, 3, False)],
                         ids=["M24-fused", "M100-fused-first-RHF", "M120-stacked"])
def test_the_window_is_read_only_on_the_walk(shape):
    """Two handles with the same walkers and fields, one closes a window between steps: walkers, Ghalf, G, the
    determinant weights and the next two steps are bitwise equal."""
    M, K, na, nb, nw, rhf = shape
    devs = [Case(M, K, na, nb, 3, nw, rhf_first=rhf) for _ in range(2)]
    a, b = devs
    rng = numpy.random.RandomState(17)
    for c in devs:
        c.dev.bp_configure(3)
    for k in range(3):
        xi = rng.normal(size=(nw, K))
        for c in devs:
            c.dev.propagate(xi, 0.2)
    for c in devs:
        c.dev.greens(want_G=True)
    before = state(a.dev)
    assert all(numpy.array_equal(x, y) for x, y in zip(before, state(b.dev)))
    E, den, G, detw = a.dev.bp_update_msd(a.dets, a.coeffs, 2, 'full', True)
    assert numpy.isfinite(G).all() and abs(den) > 0
    assert all(numpy.array_equal(x, y) for x, y in zip(state(a.dev), before))
    for k in range(2):
        xi = rng.normal(size=(nw, K))
        for c in devs:
            c.dev.propagate(xi, 0.2)
        sa, sb = state(a.dev), state(b.dev)
        assert all(numpy.array_equal(x, y) for x, y in zip(sa, sb)), k
    for c in devs:
        c.dev.close()


def test_consecutive_windows_a_clone_inside_a_window_and_two_path_lengths():
    """Three consecutive windows on one handle; in the second a walker is cloned half way (the clone carries its
    parent's history, phi_old and weight factors); in the third the window is also evaluated at half its length
    (nsplit = 2: reset only at the full length)."""
    M, K, na, nb, nd, nw, nbp = 24, 12, 6, 5, 3, 5, 4
    c = Case(M, K, na, nb, nd, nw)
    c.dev.bp_configure(nbp)
    phi0 = c.dev.get(L.F_PHI).copy()
    xs = c.steps(nbp)
    c.window("window 1 of 3", xs, phi0, 2, 'full', True, fused=True)
    phi0 = c.dev.get(L.F_PHI).copy()
    xs = c.steps(2)
    c.dev.copy_walker(0, 3)
    phi0[3] = phi0[0]
    for x in xs:
        x[3] = x[0]
    xs += c.steps(2)
    assert list(c.dev.bp_steps()) == [nbp] * nw
    c.window("window 2 of 3, walker 3 cloned from 0 after 2 steps", xs, phi0, 2, 'full', True, fused=True)
    phi0 = c.dev.get(L.F_PHI).copy()
    xs = c.steps(2)
    c.window("window 3 of 3 at half length (nsplit 2)", xs, phi0, 1, 'partial', reset=False, fused=True)
    assert list(c.dev.bp_steps()) == [2] * nw
    xs += c.steps(2)
    c.window("window 3 of 3 at full length", xs, phi0, 1, 'partial', fused=True)
    assert list(c.dev.bp_steps()) == [0] * nw
    c.dev.close()


def test_refusals_and_a_usable_handle():
    c = Case(12, 9, 3, 3, 2, 3)
    with pytest.raises(L.AfqError) as e:
        c.dev.itcf_configure(2, 1)
    assert e.value.code == -5 and 'multi-determinant' in str(e.value)
    c.dev.bp_configure(3)
    with pytest.raises(L.AfqError) as e:
        c.dev.itcf_configure(2, 1)
    assert e.value.code == -5
    for kw in (dict(two_rdm=True), dict(ekt=True, h1=c.H1[0])):
        with pytest.raises(L.AfqError) as e:
            c.dev.bp_observables(**kw)
        assert e.value.code == -5
    with pytest.raises(L.AfqError) as e:
        c.dev.bp_update_msd(c.dets[:1], c.coeffs[:1], 2)
    assert e.value.code == -1
    phi0 = c.dev.get(L.F_PHI).copy()
    xs = c.steps(3)
    c.window("after refusals M=12 3+3", xs, phi0, 2, fused=True)
    c.dev.close()
    model, s, rng = generic_model(12, 9, 3, 3)
    dev = make_device(model, 2)
    dev.set(L.F_PHI, numpy.array([model.psi] * 2))
    dev.set(L.F_OT, dev.calc_overlap())
    dev.bp_configure(2)
    with pytest.raises(L.AfqError) as e:
        dev.bp_update_msd(numpy.array([model.psi] * 2), numpy.ones(2), 2)
    assert e.value.code == -2
    dev.close()


# ---------------------------------------------------------------------------------------------------- the drivers
NBP_TAU = 0.0405            # 4 steps of 0.01


def msd_build():
    s = systems.synthetic_generic(12, 10, (3, 3), seed=3)
    t0 = trial_mod.rhf_trial_generic(s)
    rng = numpy.random.RandomState(9)
    dets = numpy.array([t0.psi + (0.0 if d == 0 else 0.05) * (rng.rand(12, 6) + 1j * rng.rand(12, 6)) for d in range(3)])
    return s, trial_mod.MultiDetTrial(s, (numpy.array([0.8 + 0.1j, 0.3 - 0.2j, 0.2 + 0.05j]), dets), init=t0.psi)


def drive_once(batched, bp, basename):
    s, t = msd_build()
    est = {'mixed': {'energy_eval_freq': 2, 'verbose': False}, 'basename': basename}
    if bp:
        est['back_propagated'] = {'tau_bp': NBP_TAU, 'one_rdm': True, 'evaluate_energy': True, 'restore_weights': 'full'}
    options = {'qmc': {'timestep': 0.01, 'num_steps': 10, 'blocks': 2, 'stabilise_freq': 5, 'pop_control_freq': 5,
                       'num_walkers': 6, 'rng_seed': 7},
               'propagator': {'device_rng': False, 'rng_seed': 7}, 'estimators': est}
    numpy.random.seed(1234)
    afqmc = AFQMC(options=options, system=s, trial=t)
    if batched:
        afqmc.run_batched()
    else:
        afqmc.run()
    afqmc.finalise(verbose=False)
    blocks = numpy.array(afqmc.estimators.estimators['mixed'].blocks)
    phi = afqmc.psi.dev.get(L.F_PHI).copy()
    est = afqmc.estimators.estimators.get('back_prop')
    release_context(s, t)
    return blocks, phi, est


@pytest.mark.parametrize("batched", [False, True], ids=["run", "run_batched"])
def test_drivers_with_a_three_determinant_trial(tmp_path, batched):
    """AFQMC.run / run_batched with a NOMSD trial and estimators: {back_propagated}: the mixed blocks and the walkers
    are bitwise those of the run without the estimator; the file's one_rdm traces are Na and Nb."""
    from pauxy_amd.utils.io import extract_rdm
    plain, phi_plain, none = drive_once(batched, False, str(tmp_path / 'plain'))
    blocks, phi, est = drive_once(batched, True, str(tmp_path / 'bp'))
    assert none is None and est is not None
    assert numpy.array_equal(blocks[:, 1:10], plain[:, 1:10]) and numpy.array_equal(phi, phi_plain)
    assert len(est.one_rdm) == 5 and len(est.energies) == 5
    rdm = extract_rdm(str(tmp_path / 'bp.0.h5'), rdm_type='one_rdm')
    assert rdm.shape == (5, 2, 12, 12)
    for g in rdm:
        assert abs(numpy.trace(g[0]) - 3) < 1e-8 and abs(numpy.trace(g[1]) - 3) < 1e-8
    e = numpy.array(est.energies)
    assert numpy.isfinite(e).all() and rel(e[:, 0], e[:, 1] + e[:, 2]) < 1e-12


def rank_drive(comm, nw_total, first, count):
    from pauxy_amd.estimators import back_propagation as bp_mod
    got = []
    base_options, base_build = mr.options, mr.build

    def options(nw, walkers=None):
        o = base_options(nw, walkers)
        o['estimators']['mixed']['one_rdm'] = False
        o['estimators']['back_propagated'] = {'tau_bp': NBP_TAU, 'one_rdm': True, 'evaluate_energy': True}
        return o
    print_step = bp_mod.BackPropagation.print_step

    def capture(self, comm_, nprocs, step, *a, **k):
        had = self.accumulated
        print_step(self, comm_, nprocs, step, *a, **k)
        if had and (comm_ is None or comm_.rank == 0):
            got.append((step, self.one_rdm[-1] / self.denominator[-1], self.energies[-1].copy()))
    mr.options, mr.build, bp_mod.BackPropagation.print_step = options, msd_build, capture
    try:
        out = mr.drive(comm, nw_total, first, count)
    finally:
        mr.options, mr.build, bp_mod.BackPropagation.print_step = base_options, base_build, print_step
    out['bp'] = got
    return out


def _worker(rank, port, q):
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE='2', LOCAL_RANK='0')
        import torch
        import torch.distributed as dist
        from pauxy_amd.comm import TorchComm
        dist.init_process_group('gloo', rank=rank, world_size=2)
        comm = TorchComm(device=torch.device('cpu'))
        q.put((rank, rank_drive(comm, 2 * mr.NW, rank * mr.NW, mr.NW)))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:
        q.put((rank, repr(e)))
        raise


def test_two_ranks_give_the_windows_of_one_rank():
    """Two ranks of the real driver sharing the GPU (the harness of tests/test_gpu_multirank.py): walkers cloned across
    the rank boundary carry their history into open windows; the reduced sums are the one-rank ones."""
    import numpy.random as npr
    keep = npr.normal, npr.random
    try:
        one = rank_drive(None, 2 * mr.NW, 0, 2 * mr.NW)
    finally:
        npr.normal, npr.random = keep
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = mr.free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=300) for _ in procs], key=lambda x: x[0])
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
    for rank, out in res:
        assert isinstance(out, dict), (rank, out)
    a, b = res[0][1], res[1][1]
    mr.compare(one, a, b)
    assert [s for s, _, _ in a['bp']] == [s for s, _, _ in one['bp']] and len(one['bp']) == 5 and b['bp'] == []
    for (step, g1, e1), (_, g2, e2) in zip(one['bp'], a['bp']):
        print("BPMSD-RANKS | window closing at step %d | two ranks vs one: G %.2e E %.2e" % (step, rel(g2, g1), rel(e2, e1)))
        assert rel(g2, g1) < 1e-9 and rel(e2, e1) < 1e-9


# ---------------------------------------------------------------------------------------------------- C5 sizes
def test_c5_sizes_window_with_four_distinct_complex_determinants():
    """BASELINE configs[4] sizes (M=400, K=2000, 50+50) with four distinct complex determinants: one window over the 4
    walkers and 3 recorded steps of tests/test_gpu_fullsize.py::test_c5_sizes_back_propagation_window, all four
    walkers against the extended restatement (dealt over worker processes)."""
    M, K, N, dt, nw, nbp, nd = 400, 2000, 50, 0.005, 4, 3, 4
    s = systems.synthetic_generic(M, K, (N, N), seed=7)
    t0 = trial_mod.rhf_trial_generic(s)
    rng = numpy.random.RandomState(3)
    dets = numpy.array([t0.psi + (0.0 if d == 0 else 0.05) * (rng.rand(M, 2 * N) + 1j * rng.rand(M, 2 * N)) for d in range(nd)])
    coeffs = numpy.array([0.8 + 0.1j, 0.3 - 0.2j, 0.2 + 0.05j, -0.1 + 0.15j])
    t = trial_mod.MultiDetTrial(s, (coeffs, dets), init=t0.psi)
    BH1, mf = setup.generic_propagator_arrays(s, t, dt)
    rng = numpy.random.RandomState(11)
    phis = t0.psi[None] + 0.05 * (rng.rand(nw, M, 2 * N) + 1j * rng.rand(nw, M, 2 * N))
    dev = AfqDevice(0)
    per = M * 2 * N
    dev.set_system_generic(s.hs_pot, t._rchol[:per], s.H1.astype(complex), s.ecore, N, N)
    dev.set_trial_multi(dets, coeffs, t._rchol)
    dev.set_propagator(BH1, mf, dt)
    dev.walkers_alloc(nw)
    dev.set(L.F_PHI, phis)
    dev.set(L.F_OT, dev.calc_overlap())
    dev.bp_configure(nbp)
    xs = []
    for step in range(nbp):
        dev.propagate(rng.normal(size=(nw, K)), 0.1)
        xs.append(dev.get(L.F_XSHIFTED).copy())
    wt = dev.get(L.F_WEIGHT).astype(complex)
    dev.launch_trace(True)
    got = dev.bp_update_msd(dets, coeffs, 2)
    trace = dev.launch_trace_get()
    dev.launch_trace(False)
    assert count(trace, VHS) == nbp and has(trace, 'k_bp_msd_taylor: stacked GEMM'), trace
    R.compare("C5 sizes M=400 K=2000 50+50 ndet=4", got, numpy.asarray(s.hs_pot), BH1, dt, numpy.array(xs), phis, dets,
              coeffs, N, 2, wt, path='stacked GEMM chain, V built %d x' % count(trace, VHS))
    dev.close()
