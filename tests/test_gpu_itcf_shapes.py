"""The ITCF window (afq_itcf_configure / afq_itcf_update) on the paths and edges its production kernels dispatch over,
and through sequences on one handle.  Every window is compared with the extended-precision restatement of the histories
recorded from the device (F_XSHIFTED per step, or the Hirsch fields) under the rule of tests/itcf_ref_ext.py
(itcf_models.compare_window): a bound per case from the fp64 restatement's own distance to the extended one.

The kernel a case is meant to reach is named in its id and asserted from the launch trace of the update (or the
library's counters), so that a later change of a dispatch threshold cannot silently empty the case:
  greens   tiny / small / lds / blocked / fallback: greens_tiny_kernel, greens_small_kernel<.., true> (up to 32 electrons
           per spin), greens_small_kernel<.., false> (33 .. 45 while walker and overlap matrices fit 160 KB of LDS),
           k_greens_big with the blocked Gauss-Jordan gj_mfma_kernel, greens_kernel -- all with a per-walker trial
  fused    the backward pass runs prop_fused_kernel (True) or the GEMM chain (False: M > 104, more than 32 electrons per
           spin, or nb == 0)
  closed   afq_counters [3]: the backward pass took the fused propagator's closed-shell deal
Which VHS builder runs (ring engine above 32 walkers) is decided by the walker count alone and has no name of its own
in the trace.  Every shape here first takes plain steps through afq_propagate (which refuses what it cannot run); the
window itself then pins the recorded fields and the weights of those steps."""
import numpy
import pytest

from oracle import afqmc_ref as ref
from pauxy_amd import _lib as L, trial as trial_mod
from pauxy_amd.qmc.afqmc import AFQMC
from pauxy_amd.utils.io import extract_mixed_estimates
from tests.helpers import make_device
from tests.itcf_models import compare_window, generic_model, hirsch_device, restore_factors

pytestmark = pytest.mark.gpu

GREENS = {'tiny': ['greens_tiny_kernel<true>'], 'small': ['greens_small_kernel<true, true>'],
          'lds': ['greens_small_kernel<true, false>'], 'blocked': ['k_greens_big: OvlpProb GEMM', 'gj_mfma_kernel'],
          'fallback': None}
EVERY_GREENS = ['greens_tiny_kernel', 'greens_small_kernel', 'k_greens_big', 'gj_mfma_kernel']


def has(names, sub):
    return any(sub in n for n in names)


def traced_update(dev, psi_T, nstblz, greens=None, fused=None, closed=None):
    """afq_itcf_update under the launch trace -> ((spgf, den), the path that was asserted, in words)."""
    dev.launch_trace(True)
    before = dev.counters(n=8).copy()
    got = dev.itcf_update(psi_T, nstblz)
    names = set(dev.launch_trace_get())
    dev.launch_trace(False)
    took = dev.counters(n=8) - before
    said = []
    if greens is not None:
        if GREENS[greens] is None:                       # the general kernel: its bare name, and none of the others
            assert any(n.strip('()') == 'greens_kernel' for n in names), sorted(names)
            assert not any(has(names, k) for k in EVERY_GREENS), sorted(names)
        else:
            for k in GREENS[greens]:
                assert has(names, k), (k, sorted(names))
            assert not any(n.strip('()') == 'greens_kernel' for n in names), sorted(names)
            if greens != 'blocked':
                assert not has(names, 'k_greens_big'), sorted(names)
        said.append('greens: ' + greens)
    if fused is not None:
        assert has(names, 'prop_fused_kernel') == fused, sorted(names)
        said.append('backward pass: ' + ('prop_fused_kernel' if fused else 'GEMM chain'))
    if closed is not None:
        assert (int(took[3]) > 0) == closed, took
        said.append('closed-shell deal: %d walker steps' % int(took[3]))
    assert has(names, 'itcf_accumulate_kernel') and has(names, 'itcf_weights_kernel')
    return got, ', '.join(said)


# ---------------------------------------------------------------------------------------------------- Generic
def generic_device(M, K, na, nb, nw, hermitian=False, rhf=False, opened=(), dead=(), seed=3):
    model, s, rng = generic_model(M, K, na, nb, seed, hermitian=hermitian, rhf=rhf)
    dev = make_device(model, nw)
    ne = na + nb
    if rhf:                                              # walkers exactly at the trial: spin blocks bitwise equal
        phi = numpy.array([model.psi] * nw)
        for w in opened:
            phi[w][:, na:] += 0.05 * (rng.rand(M, nb) + 1j * rng.rand(M, nb))
    else:
        phi = numpy.array([model.psi + 0.1 * (rng.rand(M, ne) + 1j * rng.rand(M, ne)) for _ in range(nw)])
    dev.set(L.F_PHI, phi)
    dev.set(L.F_OT, dev.calc_overlap())
    if len(dead):
        w = dev.get(L.F_WEIGHT).copy()
        w[list(dead)] = 0.0
        dev.set(L.F_WEIGHT, w)
    return dev, model, s, rng


def generic_steps(dev, rng, K, n):
    xs = []
    for step in range(n):
        dev.propagate(rng.normal(size=(dev.nw, K)), 0.2)
        xs.append(dev.get(L.F_XSHIFTED).copy())
    return xs


def generic_window(case, dev, model, s, xs, phi0, na, nmax, nstblz, stable, restore=False, sample=False, **path):
    wfac = restore_factors(dev, model.psi, nstblz) if restore else dev.get(L.F_WEIGHT).astype(complex)
    got, said = traced_update(dev, model.psi, nstblz, **path)
    return compare_window(case, got, 'generic', (numpy.asarray(s.hs_pot), numpy.asarray(model.BH1), model.dt),
                          numpy.array(xs), phi0, model.psi, na, nmax, nstblz, stable, wfac, sample=sample, path=said)


def run_generic(case, M, K, na, nb, nw, nmax=3, neqlb=1, nstblz=1, stable=True, restore=False, sample=False, hermitian=False,
                rhf=False, opened=(), dead=(), seed=3, **path):
    dev, model, s, rng = generic_device(M, K, na, nb, nw, hermitian, rhf, opened, dead, seed)
    dev.itcf_configure(nmax, neqlb, stable, restore)
    phi0 = dev.get(L.F_PHI).copy()
    if rhf:
        closed = numpy.array([numpy.array_equal(p[:, :na], p[:, na:]) for p in phi0])
        assert closed.sum() == nw - len(opened)
    xs = generic_steps(dev, rng, K, nmax + neqlb)
    w = dev.get(L.F_WEIGHT)
    assert all(w[d] == 0 for d in dead) and numpy.isfinite(w).all()
    if rhf:                                              # closed walkers stay closed through the steps, bit for bit
        after = dev.get(L.F_PHI)
        assert all(numpy.array_equal(p[:, :na], p[:, na:]) == c for p, c in zip(after, closed))
    out = generic_window(case, dev, model, s, xs, phi0, na, nmax, nstblz, stable, restore, sample, **path)
    dev.close()
    return out


def third(nw):
    return tuple(range(1, nw, 3))


CLOSED = [
    # M=100, 25+25, RHF real trial: the benchmark's configuration; Green's function of 25 electrons per spin, fused
    # backward pass in the closed-shell deal.  64 and 256 walkers are referenced through a four-walker sample.
    ("closed M=100 25+25 nw=8 [small, fused, closed deal]", dict(M=100, K=20, na=25, nb=25, nw=8, rhf=True, greens='small', fused=True, closed=True)),
    ("closed M=100 25+25 nw=64 [small, fused, closed deal; ring VHS; sampled]", dict(M=100, K=20, na=25, nb=25, nw=64, nmax=2, rhf=True, sample=True, greens='small', fused=True, closed=True)),
    ("closed M=100 25+25 nw=256 [small, fused, closed deal; ring VHS; sampled]", dict(M=100, K=20, na=25, nb=25, nw=256, nmax=2, rhf=True, sample=True, greens='small', fused=True, closed=True)),
    ("mixed M=100 25+25 nw=8, a third open, two dead [small, fused, closed deal]", dict(M=100, K=20, na=25, nb=25, nw=8, rhf=True, opened=third(8), dead=(0, 5), greens='small', fused=True, closed=True)),
    ("mixed M=100 25+25 nw=256, a third open, two dead [sampled]", dict(M=100, K=20, na=25, nb=25, nw=256, nmax=2, rhf=True, opened=third(256), dead=(7, 200), sample=True, greens='small', fused=True, closed=True)),
    ("mixed M=100 25+25 nw=64, a third open, two dead, unstable [sampled]", dict(M=100, K=20, na=25, nb=25, nw=64, nmax=2, stable=False, rhf=True, opened=third(64), dead=(0, 41), sample=True, greens='small', fused=True, closed=True)),
    ("closed M=40 13+13 nw=6 [small, fused]", dict(M=40, K=16, na=13, nb=13, nw=6, nmax=4, nstblz=2, rhf=True, greens='small', fused=True)),
    ("closed (H) M=64 32+32 nw=4 [small, fused]", dict(M=64, K=16, na=32, nb=32, nw=4, rhf=True, hermitian=True, greens='small', fused=True)),
]

GREENS_CLASSES = [
    # M=100 with 40+37: walker and overlap matrices (177 KB) do not fit the LDS kernel, so the blocked path takes it;
    # M=64 with 40+37 is the 33 .. 45 class of the LDS kernel
    ("M=100 40+37 [blocked Gauss-Jordan, GEMM chain]", dict(M=100, K=12, na=40, nb=37, nw=3, greens='blocked', fused=False)),
    ("M=64 40+37 [lds 33..45, GEMM chain]", dict(M=64, K=12, na=40, nb=37, nw=3, greens='lds', fused=False)),
    ("M=100 45+45 [blocked Gauss-Jordan, GEMM chain]", dict(M=100, K=12, na=45, nb=45, nw=3, greens='blocked', fused=False)),
    ("M=128 64+64 [blocked Gauss-Jordan, GEMM chain]", dict(M=128, K=12, na=64, nb=64, nw=2, nmax=2, greens='blocked', fused=False)),
    ("M=64 50+0 [greens_kernel fallback, GEMM chain]", dict(M=64, K=12, na=50, nb=0, nw=3, greens='fallback', fused=False)),
    ("M=24 8+8 [tiny, fused]", dict(M=24, K=12, na=8, nb=8, nw=4, greens='tiny', fused=True)),
    ("M=24 9+8 [small, fused]", dict(M=24, K=12, na=9, nb=8, nw=4, greens='small', fused=True)),
    ("M=48 16+17 [small, fused]", dict(M=48, K=12, na=16, nb=17, nw=3, greens='small', fused=True)),
    ("M=16 16+15 filled band [small, fused]", dict(M=16, K=12, na=16, nb=15, nw=4, greens='small', fused=True)),
]

BACKWARD = [
    ("M=105 20+19 [GEMM chain]", dict(M=105, K=12, na=20, nb=19, nw=2, greens='small', fused=False)),
    ("M=120 20+19 restore [GEMM chain]", dict(M=120, K=12, na=20, nb=19, nw=2, nmax=2, restore=True, greens='small', fused=False)),
    ("M=128 20+19 unstable [GEMM chain]", dict(M=128, K=12, na=20, nb=19, nw=2, nmax=2, stable=False, greens='small', fused=False)),
    ("M=33 4+0 [nb == 0: GEMM chain, tiny]", dict(M=33, K=12, na=4, nb=0, nw=3, nmax=4, nstblz=2, greens='tiny', fused=False)),
    ("M=6 2+0 [nb == 0: GEMM chain, tiny]", dict(M=6, K=5, na=2, nb=0, nw=3, greens='tiny', fused=False)),
    ("M=37 6+7 na < nb [fused, tiny]", dict(M=37, K=12, na=6, nb=7, nw=3, greens='tiny', fused=True)),
]


def edge(M):
    na = max(1, min(5, M // 2))
    return ("M=%d %d+%d" % (M, na, max(1, na - 1)),
            dict(M=M, K=9, na=na, nb=max(1, na - 1), nw=2 + M % 4, nmax=3 if M < 90 else 2, fused=M <= 104))


GEMM_EDGES = [edge(M) for M in (2, 3, 8, 9, 17, 24, 31, 32, 33, 63, 65, 97, 127)] + [
    ("M=64 nw=33 [ring VHS]", dict(M=64, K=12, na=7, nb=5, nw=33, nmax=2, fused=True)),
    ("M=64 nw=64 [ring VHS]", dict(M=64, K=12, na=7, nb=5, nw=64, nmax=2, dead=(63,), fused=True)),
    ("M=64 nw=65 unstable [ring VHS]", dict(M=64, K=12, na=7, nb=5, nw=65, nmax=2, stable=False, fused=True)),
    ("(H) M=100 nw=33 [ring VHS]", dict(M=100, K=12, na=7, nb=5, nw=33, nmax=2, hermitian=True, fused=True)),
    ("(H) M=100 nw=64 [ring VHS; sampled]", dict(M=100, K=12, na=7, nb=5, nw=64, nmax=2, hermitian=True, sample=True, fused=True)),
    ("(H) M=100 nw=65 [ring VHS; sampled]", dict(M=100, K=12, na=7, nb=5, nw=65, nmax=2, hermitian=True, dead=(0, 64), sample=True, fused=True)),
    ("M=16 nw=257 [weights: strided loop]", dict(M=16, K=12, na=5, nb=3, nw=257, nmax=2, dead=(0, 255, 256), fused=True)),
    ("M=16 nw=1000 [weights: strided loop]", dict(M=16, K=12, na=5, nb=3, nw=1000, nmax=2, dead=tuple(range(3, 1000, 7)), fused=True)),
]

WINDOW = [
    ("nmax=1 unstable: B and B^-1 alone", dict(nmax=1, neqlb=0, stable=False, nw=1)),
    ("nmax=1 stable", dict(nmax=1, neqlb=2, nstblz=1)),
    ("neqlb=0", dict(nmax=5, neqlb=0, nstblz=2)),
    ("neqlb=3 nmax", dict(nmax=2, neqlb=6, nstblz=3)),
    ("nstblz=1", dict(nmax=5, neqlb=1, nstblz=1)),
    ("nstblz >= nmax + neqlb: never re-orthogonalised", dict(nmax=4, neqlb=2, nstblz=6)),
    ("restore on, unstable", dict(nmax=4, neqlb=1, nstblz=2, stable=False, restore=True)),
    ("restore on, stable", dict(nmax=4, neqlb=1, nstblz=2, restore=True)),
]


def params(rows):
    return [pytest.param(case, kw, id=case.replace(' ', '_')) for case, kw in rows]


@pytest.mark.parametrize("case,kw", params(CLOSED))
def test_closed_shell_populations(case, kw):
    run_generic(case, **kw)


@pytest.mark.parametrize("case,kw", params(GREENS_CLASSES))
def test_greens_function_classes_with_a_per_walker_trial(case, kw):
    run_generic(case, **kw)


@pytest.mark.parametrize("case,kw", params(BACKWARD))
def test_backward_pass_off_the_fused_kernel(case, kw):
    run_generic(case, **kw)


@pytest.mark.parametrize("case,kw", params(GEMM_EDGES))
def test_gemm_tile_chunk_and_walker_count_edges(case, kw):
    run_generic(case, **kw)


@pytest.mark.parametrize("case,kw", params(WINDOW))
def test_window_parameters(case, kw):
    kw = dict(dict(M=16, K=12, na=5, nb=3, nw=4, dead=()), **kw)
    run_generic("window " + case, fused=True, greens='tiny', **kw)


def test_filled_band_has_no_greater_function():
    """M = na = 16: P = I for that spin, Ggr = 0 to rounding at every tau (an absolute statement the rule's relative
    scale max(1, .) keeps)."""
    dev, model, s, rng = generic_device(16, 12, 16, 15, 3)
    dev.itcf_configure(3, 1, True, False)
    generic_steps(dev, rng, 12, 4)
    spgf, den = dev.itcf_update(model.psi, 2)
    assert float(numpy.max(numpy.abs(spgf[:, 0, 0]))) <= 1e-13 * abs(den)
    assert float(numpy.max(numpy.abs(spgf[0, 0, 1] - den.real * numpy.eye(16)))) <= 1e-13 * abs(den)
    dev.close()


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_handle_usable():
    from pauxy_amd import systems
    from pauxy_amd.propagation import setup
    from tests.test_gpu_sizes import build
    # M = 129: the batched Gauss-Jordan inverse of B stops at 128
    dev, model, s, rng = generic_device(129, 6, 3, 2, 2)
    with pytest.raises(L.AfqError) as e:
        dev.itcf_configure(2, 1)
    assert e.value.code == -5 and 'M > 128' in str(e.value)
    dev.propagate(rng.normal(size=(2, 6)), 0.1)
    assert numpy.isfinite(dev.get(L.F_WEIGHT)).all() and numpy.isfinite(dev.get(L.F_PHI)).all()
    dev.close()
    # general complex Cholesky vectors: B(-conj(x)) is not B(x)^H
    gmodel, grng = build(12, 8, 3, 2, True, lform='general')
    dev = make_device(gmodel, 2)
    dev.set(L.F_PHI, numpy.array([gmodel.psi] * 2))
    dev.set(L.F_OT, dev.calc_overlap())
    with pytest.raises(L.AfqError) as e:
        dev.itcf_configure(2, 1)
    assert e.value.code == -5
    dev.propagate(grng.normal(size=(2, 8)), 0.1)
    assert numpy.isfinite(dev.get(L.F_WEIGHT)).all()
    dev.close()
    # a multi-determinant trial
    M, K, na, nb, dt = 12, 9, 3, 3, 0.005
    sm = systems.synthetic_generic(M, K, (na, nb), seed=7)
    t0 = trial_mod.rhf_trial_generic(sm)
    mrng = numpy.random.RandomState(5)
    dets = numpy.array([t0.psi + 0.05 * (mrng.rand(M, na + nb) + 1j * mrng.rand(M, na + nb)) for _ in range(2)])
    coeffs = numpy.array([0.8 + 0.1j, 0.5 - 0.2j])
    t = trial_mod.MultiDetTrial(sm, (coeffs, dets), init=t0.psi)
    BH1, mf = setup.generic_propagator_arrays(sm, t, dt)
    mmodel = ref.RefModel('generic_msd', M, na, nb, dets, BH1, mf, dt, coeffs=coeffs, hs_pot=sm.hs_pot,
                          H1=numpy.array([sm.H1[0], sm.H1[1]]).astype(complex), ecore=sm.ecore)
    dev = make_device(mmodel, 2)
    dev.set(L.F_PHI, numpy.array([t0.psi] * 2))
    dev.greens(want_G=False)
    with pytest.raises(L.AfqError) as e:
        dev.itcf_configure(2, 1)
    assert e.value.code == -5
    dev.propagate(mrng.normal(size=(2, K)), 0.0)
    assert numpy.isfinite(dev.get(L.F_WEIGHT)).all()
    dev.close()
    # invalid arguments, an update without a configuration; then a valid configuration works on the same handle
    dev, model, s, rng = generic_device(16, 12, 5, 3, 3)
    for bad in ((0, 1), (2, -1)):
        with pytest.raises(L.AfqError) as e:
            dev.itcf_configure(*bad)
        assert e.value.code == -1
    with pytest.raises(L.AfqError) as e:
        dev.itcf_update(model.psi, 2)
    assert e.value.code == -2
    dev.itcf_configure(2, 1, True, False)
    phi0 = dev.get(L.F_PHI).copy()
    xs = generic_steps(dev, rng, 12, 3)
    generic_window("after refusals M=16 5+3", dev, model, s, xs, phi0, 5, 2, 2, True, fused=True, greens='tiny')
    dev.close()
    # AFQ_EUNSUPPORTED and then a valid configuration on the SAME handle: discrete fields record no weight factors, so
    # restore_weights is refused; without it the handle configures and its window is right.  (For M = 129, general
    # complex vectors and a multi-determinant trial no valid configuration exists: those handles only go on propagating.)
    dev, BT2, psi, hrng, U, hdt = hirsch_device(3, 3, 5, 4, 4)
    with pytest.raises(L.AfqError) as e:
        dev.itcf_configure(2, 1, True, True)
    assert e.value.code == -5 and 'restore_weights' in str(e.value)
    dev.itcf_configure(2, 1, True, False)
    phi0 = dev.get(L.F_PHI).copy()
    fields = hirsch_steps(dev, hrng, 3)
    hirsch_window("after a refusal, hirsch 3x3 5+4", dev, BT2, psi, U, hdt, fields, phi0, 5, 2, 2, True, greens='tiny')
    dev.close()


# ---------------------------------------------------------------------------------------------------- Hirsch
def hirsch_steps(dev, rng, n):
    fields = []
    for step in range(n):
        dev.hirsch_kinetic()
        f, _ = dev.hirsch_two_body(rng.random_sample((dev.nw, dev.M)))
        dev.hirsch_finish(0.0)
        fields.append(f)
    return fields


def hirsch_window(case, dev, BT2, psi, U, dt, fields, phi0, na, nmax, nstblz, stable, unit_weights=False, **path):
    fields = numpy.array(fields)
    if unit_weights:
        # the charge decomposition's walk leaves weights of 1e-3 and less behind, under which the rule's scale
        # max(1, max |slice|) would compare absolute errors of nothing: live walkers count with weight 1
        dev.set(L.F_WEIGHT, (dev.get(L.F_WEIGHT) != 0).astype(float))
    wfac = dev.get(L.F_WEIGHT).astype(complex)
    # a walker that died inside the window has no complete history (its later fields stay unset) and a zero weight
    wfac[(fields < 0).any(axis=(0, 2))] = 0.0
    died = wfac == 0
    got, said = traced_update(dev, psi, nstblz, **path)
    said = (said + ', ' if said else '') + '%d died inside the window' % int(died.sum())
    compare_window(case, got, 'hirsch', (BT2, dt, U), fields, phi0, psi, na, nmax, nstblz, stable, wfac, path=said)
    return int(died.sum())


HIRSCH = [
    ("hirsch 3x3 5+4", dict(nx=3, ny=3, na=5, nb=4, nw=5, nmax=4, neqlb=1, nstblz=2, greens='tiny')),
    ("hirsch 8x1 4+4 unstable", dict(nx=8, ny=1, na=4, nb=4, nw=5, nmax=4, neqlb=1, nstblz=2, stable=False, greens='tiny')),
    ("hirsch 6x6 18+17", dict(nx=6, ny=6, na=18, nb=17, nw=4, nmax=3, neqlb=1, nstblz=1, greens='small')),
    ("hirsch 10x10 45+45 [blocked Gauss-Jordan]", dict(nx=10, ny=10, na=45, nb=45, nw=3, nmax=3, neqlb=1, nstblz=1, greens='blocked')),
    ("hirsch 11x11 61+60 [blocked Gauss-Jordan]", dict(nx=11, ny=11, na=61, nb=60, nw=2, nmax=2, neqlb=1, nstblz=1, greens='blocked')),
    # the walk uses the charge decomposition (complex auxiliary fields factors); B is still built from the spin
    # decomposition's real auxf, as the reference's back-propagation does (propagation/hubbard.py:589-593, noted at
    # k_hirsch.hip for bp_hirsch_step), and so does the restatement: b_hirsch knows one auxf only
    ("hirsch 3x3 5+4 charge decomposition", dict(nx=3, ny=3, na=5, nb=4, nw=5, nmax=4, neqlb=1, nstblz=2, charge=True, greens='tiny')),
    ("hirsch 4x4 7+7 charge decomposition, unstable", dict(nx=4, ny=4, na=7, nb=7, nw=37, nmax=3, neqlb=1, nstblz=2, stable=False, charge=True, greens='tiny')),
]


@pytest.mark.parametrize("case,kw", params(HIRSCH))
def test_hirsch_lattices_and_the_charge_decomposition(case, kw):
    kw = dict(kw)
    nx, ny, na, nb, nw = [kw.pop(k) for k in ('nx', 'ny', 'na', 'nb', 'nw')]
    nmax, neqlb, nstblz, stable = kw.pop('nmax'), kw.pop('neqlb'), kw.pop('nstblz'), kw.pop('stable', True)
    charge = kw.pop('charge', False)
    dev, BT2, psi, rng, U, dt = hirsch_device(nx, ny, na, nb, nw, charge_decomposition=charge)
    dev.itcf_configure(nmax, neqlb, stable, False)
    phi0 = dev.get(L.F_PHI).copy()
    fields = hirsch_steps(dev, rng, nmax + neqlb)
    hirsch_window(case, dev, BT2, psi, U, dt, fields, phi0, na, nmax, nstblz, stable, unit_weights=charge, **kw)
    dev.close()


def test_hirsch_walkers_that_die_inside_the_window():
    """U = 8, dt = 0.1 and walkers far from the trial (a third of them start with a negative overlap): the constraint
    kills three of the 64 within the window (the CPU oracle's walk of the same fields says so).  A walker that died has
    an incomplete history and does not count; the others do, and the denominator says which."""
    nw, nmax, neqlb = 64, 5, 3
    dev, BT2, psi, rng, U, dt = hirsch_device(4, 4, 7, 5, nw, U=8.0, dt=0.1)
    phi = dev.get(L.F_PHI)
    phi += 1.5 * (rng.rand(*phi.shape) - 0.5)
    dev.set(L.F_PHI, phi)
    dev.set(L.F_OT, dev.calc_overlap())
    dev.itcf_configure(nmax, neqlb, True, False)
    phi0 = dev.get(L.F_PHI).copy()
    fields = hirsch_steps(dev, rng, nmax + neqlb)
    died = hirsch_window("hirsch 4x4 7+5 U=8 nw=64, walkers die", dev, BT2, psi, U, dt, fields, phi0, 7, nmax, 2, True,
                         greens='tiny')
    assert 1 <= died < nw, died
    dev.close()


# ---------------------------------------------------------------------------------------------------- sequences
def test_three_consecutive_windows_generic():
    """History reset and phi_old refreshed by every update: each window against the restatement started from the
    device's walkers at that window's start."""
    M, K, na, nb, nw, nmax, neqlb, nstblz = 24, 12, 6, 5, 6, 3, 1, 2
    dev, model, s, rng = generic_device(M, K, na, nb, nw, dead=(2,))
    dev.itcf_configure(nmax, neqlb, True, False)
    for k in range(3):
        phi0 = dev.get(L.F_PHI).copy()
        xs = generic_steps(dev, rng, K, nmax + neqlb)
        generic_window("window %d of 3, generic M=24 6+5" % (k + 1), dev, model, s, xs, phi0, na, nmax, nstblz, True,
                       fused=True, greens='tiny')
        if k == 0:
            dev.reortho()                                # the walk goes on between windows as a driver's would
    dev.close()


@pytest.mark.parametrize("stable", [True, False])
def test_three_consecutive_windows_hirsch(stable):
    """The discrete history counts single fields (bp_n % M): three windows in a row on one handle."""
    nmax, neqlb, nstblz = 3, 2, 2
    dev, BT2, psi, rng, U, dt = hirsch_device(3, 3, 5, 4, 6)
    dev.itcf_configure(nmax, neqlb, stable, False)
    for k in range(3):
        phi0 = dev.get(L.F_PHI).copy()
        fields = hirsch_steps(dev, rng, nmax + neqlb)
        hirsch_window("window %d of 3, hirsch 3x3 5+4 %s" % (k + 1, 'stable' if stable else 'unstable'), dev, BT2, psi, U,
                      dt, fields, phi0, 5, nmax, nstblz, stable, greens='tiny')
    dev.close()


@pytest.mark.parametrize("combs,restore", [(1, False), (2, False), (2, True)])
def test_a_comb_inside_the_window(combs, restore):
    """popcontrol_comb between the steps of a window, weights spread so that walkers are cloned and killed: a clone
    carries its parent's fields, phi_old and weight factors up to the comb and its own afterwards.  The lineage is
    replayed from the returned multiplicities (the reference pairs the walkers to clone with those to kill in order,
    walkers/handler.py:295-301).  With restore, the weight factors are read back through the back-propagation's
    denominator of each walker alone (restore_factors): they share the device's history with the window, so that case
    pins the Green's functions and the pairing of factor and walker, not the factors themselves."""
    M, K, na, nb, nw, nmax, neqlb, nstblz = 16, 12, 5, 3, 12, 4, 2, 2
    dev, model, s, rng = generic_device(M, K, na, nb, nw)
    dev.itcf_configure(nmax, neqlb, True, restore)
    phi0 = dev.get(L.F_PHI).copy()
    xs = []
    at = {1: (3,), 2: (2, 4)}[combs]
    moved = 0
    for step in range(nmax + neqlb):
        if step in at:
            w = dev.get(L.F_WEIGHT).copy()
            w *= numpy.array([2.6, 0.05, 1.0, 0.3, 3.1, 0.02, 1.0, 0.6, 0.01, 1.7, 1.0, 0.4])[(numpy.arange(nw) + step) % nw]
            dev.set(L.F_WEIGHT, w)
            pix, _ = dev.popcontrol_comb(float(rng.rand()), nw)
            pairs = ref.comb_pairs(pix)
            assert pairs and (pix == 0).any() and (pix > 1).any()
            for src, dst in pairs:
                phi0[dst] = phi0[src]
                for x in xs:
                    x[dst] = x[src]
            moved += len(pairs)
        xs += generic_steps(dev, rng, K, 1)
    assert moved >= combs
    generic_window("comb x%d inside the window M=16 5+3 nw=12%s" % (combs, ' restore' if restore else ''), dev, model, s,
                   xs, phi0, na, nmax, nstblz, True, restore, fused=True, greens='tiny')
    dev.close()


WALK = (L.F_PHI, L.F_WEIGHT, L.F_OT, L.F_DETR, L.F_HYBRID_ENERGY)


def walk(dev):
    return [dev.get(f).copy() for f in WALK]


def same(a, b):
    return all(numpy.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("split,reortho", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("shape", [(16, 12, 5, 3, 5, False), (100, 20, 25, 25, 40, True)])
def test_the_window_is_read_only_on_the_walk(shape, split, reortho):
    """Two handles with the same walkers and fields, one of them runs afq_itcf_update between steps (it writes the
    window's Green's functions into buffers of its own, builds VHS into the handle's buffer and borrows phi, ot and
    detR for the re-orthogonalisation): the walkers, and the handle's Ghalf and G (walker state of the mixed one_rdm,
    which every estimator update accumulates and the comb carries), are bitwise the same before and after the update;
    estimator updates without an energy evaluation behind the window add the same one_rdm terms; and after the next
    two steps on both handles (with and without a re-orthogonalisation in front of them, as a driver's stabilise_freq
    brings), through afq_propagate and through afq_propagate_begin / afq_propagate_finish."""
    M, K, na, nb, nw, rhf = shape
    devs = []
    for k in range(2):
        dev, model, s, rng = generic_device(M, K, na, nb, nw, rhf=rhf, opened=(1, 4) if rhf else ())
        devs.append(dev)
    a, b = devs
    a.itcf_configure(3, 1, True, False)
    b.bp_configure(4)                                    # the same history is recorded on both; only a closes a window
    for d in devs:
        d.estimates_rdm(True)
    rng = numpy.random.RandomState(17)

    def step(xi):
        for d in devs:
            if split:
                d.propagate_begin(xi)
                d.propagate_finish(0.2)
            else:
                d.propagate(xi, 0.2)
    for k in range(4):
        step(rng.normal(size=(nw, K)))
    assert same(walk(a), walk(b))
    for d in devs:
        d.estimates_update(True)                         # refreshes walker.G and accumulates it
        d.estimates_get(zero=True)
    before = walk(a) + [a.get(L.F_GHALF).copy(), a.get(L.F_G).copy()]
    assert numpy.abs(before[-1]).max() > 0 and same(before, walk(b) + [b.get(L.F_GHALF), b.get(L.F_G)])
    assert numpy.array_equal(a.estimates_rdm_get(zero=True), b.estimates_rdm_get(zero=True))
    spgf, den = a.itcf_update(model.psi, 2)
    assert numpy.isfinite(spgf).all() and abs(den) > 0
    assert same(walk(a) + [a.get(L.F_GHALF), a.get(L.F_G)], before)
    for d in devs:
        d.estimates_update(False)                        # no energy: walker.G is accumulated as it stands
        d.estimates_get(zero=True)
    ra, rb = a.estimates_rdm_get(zero=True), b.estimates_rdm_get(zero=True)
    assert numpy.abs(ra).max() > 0 and numpy.array_equal(ra, rb)
    for k in range(2):
        if k == 0 and reortho:
            # Ghalf does not change under the re-orthogonalisation, so the library keeps the one the last step left; a
            # window that dropped it made this step recompute it from the new phi, one rounding away
            for d in devs:
                d.reortho()
            assert same(walk(a), walk(b))
        step(rng.normal(size=(nw, K)))
        wa, wb = walk(a), walk(b)
        assert same(wa, wb), [int(not numpy.array_equal(x, y)) for x, y in zip(wa, wb)]
    ea, eb = a.local_energy(), b.local_energy()
    assert numpy.array_equal(ea, eb)
    for d in devs:
        d.estimates_update(True)
        d.estimates_get(zero=True)
    assert numpy.array_equal(a.estimates_rdm_get(zero=True), b.estimates_rdm_get(zero=True))
    a.close()
    b.close()


@pytest.mark.parametrize("one_rdm", [False, True])
@pytest.mark.parametrize("batched", [False, True])
def test_driver_blocks_do_not_depend_on_the_itcf(tmp_path, batched, one_rdm):
    """AFQMC.run / AFQMC.run_batched with and without the itcf block: the mixed estimator's blocks are bitwise equal,
    and with one_rdm so are its one-body RDM blocks (the device accumulates weight * walker.G with every estimator
    update, the energy is evaluated -- and walker.G refreshed -- once per block only: a window that left its own G in
    the handle would be accumulated instead)."""
    model, s, rng = generic_model(12, 16, 4, 3)
    dt = 0.01
    out, rdm = {}, {}
    for name in ('plain', 'itcf'):
        t = trial_mod.SingleDetTrial(s, model.psi)
        est = {'basename': str(tmp_path / name)}
        if name == 'itcf':
            est['itcf'] = {'tau_max': 2.5 * dt, 'tau_eqlb': 1.5 * dt, 'mode': 'full', 'restore_weights': False}
        if one_rdm:
            est['mixed'] = {'one_rdm': True}
        options = {'qmc': {'timestep': dt, 'num_steps': 3, 'blocks': 4, 'stabilise_freq': 2, 'pop_control_freq': 2,
                           'num_walkers': 6, 'rng_seed': 7},
                   'estimators': est}
        afqmc = AFQMC(options=options, system=s, trial=t)
        mixed = afqmc.estimators.estimators['mixed']
        assert bool(mixed.calc_one_rdm) == one_rdm
        if batched:
            afqmc.run_batched()
        else:
            afqmc.run(verbose=False)
        afqmc.finalise(verbose=False)
        if name == 'itcf':
            assert len(afqmc.estimators.estimators['itcf'].windows) == 4
        out[name] = extract_mixed_estimates(str(tmp_path / (name + '.0.h5')))
        rdm[name] = numpy.array(mixed.one_rdm)
    assert set(out['plain']) == set(out['itcf'])
    for k in out['plain']:
        if k.lower() == 'time':
            continue
        assert len(out['plain'][k]) >= 4
        assert numpy.array_equal(out['plain'][k], out['itcf'][k]), (k, out['plain'][k], out['itcf'][k])
    if one_rdm:
        assert rdm['plain'].shape == (4, 2, 12, 12) and numpy.isfinite(rdm['plain']).all()
        assert abs(numpy.trace(rdm['plain'][-1][0]) - 4) <= 1e-8 and abs(numpy.trace(rdm['plain'][-1][1]) - 3) <= 1e-8
        assert numpy.array_equal(rdm['plain'], rdm['itcf'])
