"""Back-propagated two-body RDM and EKT Fock matrices on the device (afq_bp_observables / afq_bp_update_ext,
k_bp_obs.hip): trajectories of the genuine reference replayed through both driver loops (make_golden_bp_obs.py), and
the device's sums against the numpy restatement (tests/bp_obs_ref.py) on per-walker back-propagated Green's functions
at larger sizes and on the kernels' dispatch boundaries."""
import numpy
import pytest

from pauxy_amd import _lib as L, systems, trial as trial_mod
from pauxy_amd.propagation import setup
from pauxy_amd.qmc.afqmc import AFQMC
from pauxy_amd.utils.io import extract_rdm
from oracle import afqmc_ref as ref
from tests import bp_obs_ref
from tests.helpers import make_device
from tests.test_gpu_traj import close, replay, run_hirsch

pytestmark = pytest.mark.gpu
TOL = 1e-8


def capture_bp(monkeypatch):
    """The driver's back-propagation estimator, kept when the run finalises."""
    got = {}
    fin = AFQMC.finalise

    def finalise(self, *a, **k):
        got['est'] = self.estimators.estimators.get('back_prop')
        return fin(self, *a, **k)
    monkeypatch.setattr(AFQMC, 'finalise', finalise)
    return got


def check_windows(est, d, sfx='', sel=None):
    sel = slice(None) if sel is None else sel
    close(numpy.array(est.denominator)[sel], d['bp_denominator' + sfx])
    if 'bp_one_rdm' + sfx in d:
        close(numpy.array(est.one_rdm)[sel], d['bp_one_rdm' + sfx])
    if 'bp_fock_1p' + sfx in d:
        close(numpy.array(est.fock_1p)[sel], d['bp_fock_1p' + sfx])
        close(numpy.array(est.fock_1h)[sel], d['bp_fock_1h' + sfx])
    if 'bp_two_rdm_samp' + sfx in d:
        two = numpy.array(est.two_rdm)[sel]
        close(two.reshape(len(two), -1)[:, d['bp_two_rdm_idx']], d['bp_two_rdm_samp' + sfx])
        if 'bp_two_rdm_full' + sfx in d:
            full = d['bp_two_rdm_full' + sfx]
            close(two[:len(full)], full)


def generic_case(d):
    na, nb = [int(x) for x in d['nelec']]
    s = systems.Generic((na, nb), numpy.array([d['h1e'], d['h1e']]), d['chol'], float(d['ecore']))
    return s, trial_mod.SingleDetTrial(s, d['psi'])


@pytest.mark.parametrize("batched", [False, True])
def test_traj_generic_two_rdm_and_ekt(golden, monkeypatch, tmp_path, batched):
    d = golden('bp_obs_generic.npz')
    s, t = generic_case(d)
    got = capture_bp(monkeypatch)
    bp = {'tau_bp': 0.025, 'one_rdm': True, 'two_rdm': True, 'evaluate_ekt': True}
    replay(d, s, t, {}, monkeypatch, est_extra={'back_propagated': bp, 'basename': str(tmp_path / 'estimates')},
           batched=batched)
    est = got['est']
    check_windows(est, d)
    fn = str(tmp_path / 'estimates.0.h5')
    den = numpy.array(est.denominator)
    for kind in ('fock_1p', 'fock_1h', 'two_rdm'):
        want = numpy.array(getattr(est, kind))
        assert numpy.array_equal(extract_rdm(fn, rdm_type=kind), want / den.reshape((-1,) + (1,) * (want.ndim - 1)))


def test_traj_generic_two_path_lengths(golden, monkeypatch):
    d = golden('bp_obs_split.npz')
    s, t = generic_case(d)
    for batched in (False, True):
        got = capture_bp(monkeypatch)
        bp = {'tau_bp': 0.03, 'one_rdm': True, 'two_rdm': True, 'evaluate_ekt': True, 'nsplit': 2}
        replay(d, s, t, {}, monkeypatch, est_extra={'back_propagated': bp}, batched=batched)
        est = got['est']
        sp = numpy.array(est.split_of)
        for k in (3, 6):
            check_windows(est, d, '_%d' % k, sp == k)


def test_traj_generic_ekt_offset_without_one_rdm(golden, monkeypatch):
    """one_rdm: False -- the reference reads the Fock matrices from the region of the one-body RDM."""
    d = golden('bp_obs_quirk.npz')
    s, t = generic_case(d)
    got = capture_bp(monkeypatch)
    replay(d, s, t, {}, monkeypatch, est_extra={'back_propagated': {'tau_bp': 0.025, 'one_rdm': False,
                                                                   'evaluate_ekt': True}})
    check_windows(got['est'], d)


def test_traj_ueg_two_rdm_and_ekt(golden, monkeypatch):
    d = dict(golden('traj_bp_ueg.npz'))
    d.update(golden('bp_obs_ueg.npz'))
    s = systems.UEG(float(d['sys_rs']), 7, 7, float(d['sys_ecut']))
    t = trial_mod.hartree_fock_ueg(s)
    for batched in (False, True):
        got = capture_bp(monkeypatch)
        bp = {'tau_bp': 0.04, 'one_rdm': True, 'two_rdm': True, 'evaluate_ekt': True}
        replay(d, s, t, {}, monkeypatch, est_extra={'back_propagated': bp}, batched=batched)
        check_windows(got['est'], d)


def test_traj_hirsch_two_rdm(golden, monkeypatch):
    for batched in (False, True):
        got = capture_bp(monkeypatch)
        run_hirsch(golden, monkeypatch, 'bp_obs_hirsch.npz', batched=batched,
                   bp={'tau_bp': 0.04, 'one_rdm': True, 'two_rdm': True})
        check_windows(got['est'], golden('bp_obs_hirsch.npz'))


# ---------------------------------------------------------------- device sums against the restatement
def build(M, K, na, nb, seed=5, dt=0.01, sym=True):
    """sym=False: real Cholesky vectors that are not symmetric (the EKT's L^T panels on the handle's real vectors)."""
    rng = numpy.random.RandomState(seed)
    h = rng.normal(size=(M, M))
    h1e = 0.5 * (h + h.T) - 2.0 * numpy.eye(M)
    A = rng.normal(size=(K, M, M)) * (0.3 / numpy.sqrt(M))
    Lv = 0.5 * (A + A.transpose(0, 2, 1)) if sym else 0.5 * A
    chol = numpy.ascontiguousarray(Lv.reshape(K, M * M).T)
    s = systems.Generic((na, nb), numpy.array([h1e, h1e]), chol, ecore=0.1)
    e, v = numpy.linalg.eigh(h1e)
    psi = numpy.zeros((M, na + nb), dtype=complex)
    psi[:, :na] = v[:, :na]
    psi[:, na:] = v[:, :nb]
    psi = psi + 0.05 * (rng.rand(M, na + nb) + 1j * rng.rand(M, na + nb))
    t = trial_mod.SingleDetTrial(s, psi)
    BH1, mf = setup.generic_propagator_arrays(s, t, dt)
    model = ref.RefModel('generic', M, na, nb, t.psi, BH1, mf, dt, hs_pot=s.hs_pot, rchol=t._rchol,
                         H1=s.H1.astype(complex), ecore=0.1)
    return model, h1e, Lv, rng


def run_case(M, K, na, nb, nw, two, ekt, nbp=3, restore=None, zero=(), own_L=True, nL=None, seed=5, sym=True,
             chunks=None):
    model, h1e, Lv, rng = build(M, K, na, nb, seed, sym=sym)
    dev = make_device(model, nw)
    ne = na + nb
    dev.set(L.F_PHI, numpy.array([model.psi + 0.1 * (rng.rand(M, ne) + 1j * rng.rand(M, ne)) for _ in range(nw)]))
    dev.set(L.F_OT, dev.calc_overlap())
    dev.bp_configure(nbp)
    for step in range(nbp):
        dev.propagate(rng.normal(size=(nw, K)), 0.2)
    if own_L:
        Lx = Lv
        dev.bp_observables(two_rdm=two, ekt=ekt, h1=h1e, L=None)
    else:
        nL = nL or K
        Lx = (rng.normal(size=(nL, M, M)) + 1j * rng.normal(size=(nL, M, M))) * (0.3 / numpy.sqrt(M))
        dev.bp_observables(two_rdm=two, ekt=ekt, h1=h1e, L=Lx)
    if chunks is not None:
        dev.bp_ekt_chunks(*chunks)
    w0 = dev.get(L.F_WEIGHT).copy()
    w0[list(zero)] = 0.0
    # every walker's G_bp and accumulation weight, one walker at a time (reset=False keeps the histories)
    Gs, wts = [], []
    for i in range(nw):
        one = numpy.zeros(nw)
        one[i] = 1.0
        dev.set(L.F_WEIGHT, one)
        _, den, G = dev.bp_update(model.psi, 5, restore, reset=False)
        Gs.append(G / den)
        wts.append(den * w0[i])
    dev.set(L.F_WEIGHT, w0)
    e0, den, G, extra = dev.bp_update(model.psi, 5, restore, reset=False, two_rdm=two, ekt=ekt)
    close(den, numpy.sum(wts), 1e-10)
    close(G, numpy.einsum('w,wsij->sij', numpy.array(wts), numpy.array(Gs)), 1e-10)
    want = bp_obs_ref.window(h1e, Lx, Gs, wts, two=two, ekt=ekt)
    if two:
        close(extra['two_rdm'], want[0], TOL)
    if ekt:
        close(extra['fock_1p'], want[1], TOL)
        close(extra['fock_1h'], want[2], TOL)
    # NULL extras: afq_bp_update, bitwise
    a = dev.bp_update(model.psi, 5, restore, reset=False)
    est_ext = numpy.zeros(4 + 2 * M * M, dtype=complex)
    from pauxy_amd.device import _c128, _p
    phi0 = _c128(model.psi)
    mode = {None: 0, 'partial': 1, 'full': 2}[restore]
    dev._ck(dev.lib.afq_bp_update_ext(dev.h, _p(phi0), 5, mode, 0, 0, _p(est_ext), None, None))
    assert numpy.array_equal(est_ext[4:].reshape(2, M, M), a[2]) and est_ext[3] == a[1]
    dev.close()


def test_c3_ekt_against_restatement():
    """C3 sizes: M = 100, K = 500, 25+25."""
    run_case(100, 500, 25, 25, 4, False, True)


def test_two_rdm_against_restatement():
    run_case(48, 40, 6, 5, 64, True, False)


@pytest.mark.parametrize("M,K,na,nb,nw,restore,zero,own_L,nL", [
    (23, 30, 4, 3, 5, None, (), True, None),            # odd M, Na != Nb
    (20, 25, 5, 0, 3, None, (), True, None),            # nb = 0
    (21, 30, 3, 3, 6, None, (1, 4), True, None),        # zero-weight walkers
    (22, 30, 4, 4, 4, 'partial', (), True, None),       # complex wt
    (19, 30, 3, 2, 1, None, (), True, None),            # nw = 1
    (17, 20, 3, 4, 4, 'full', (), False, 13),           # general complex L, odd nL
])
def test_dispatch_boundaries(M, K, na, nb, nw, restore, zero, own_L, nL):
    run_case(M, K, na, nb, nw, True, True, restore=restore, zero=zero, own_L=own_L, nL=nL)


@pytest.mark.parametrize("K,nL,own_L,sym,chunks", [
    (13, None, True, True, (3, 4)),         # the handle's symmetric real vectors: 4 panel chunks + 1, 3 linear + 1
    (14, None, True, False, (4, 5)),        # non-symmetric real vectors (L^T panels on L_full): 3 + 1, 2 + 1
    (20, 13, False, True, (5, 3)),          # the caller's complex vectors: 2 + 1, 4 + 1
])
def test_chunk_boundaries(K, nL, own_L, sym, chunks):
    """nL not a multiple of the chunk, for the rank-N panels and for the term linear in G."""
    run_case(21, K, 4, 3, 5, False, True, restore='partial', own_L=own_L, nL=nL, sym=sym, chunks=chunks)


def test_automatic_chunks_with_a_tail():
    """M = 40, 10+10, 64 walkers, K = 600: 2^26 elements of panel scratch hold 524 vectors, so the panels run as
    524 + 76 without any setting."""
    run_case(40, 600, 10, 10, 64, False, True)


def test_two_rdm_refused_beyond_the_memory_budget():
    model, h1e, Lv, rng = build(320, 2, 2, 2)
    dev = make_device(model, 2)
    dev.bp_configure(2)
    with pytest.raises(Exception) as e:
        dev.bp_observables(two_rdm=True)
    assert 'bytes' in str(e.value)
    dev.bp_observables(ekt=True, h1=h1e)             # the EKT alone needs no M^4 buffer
    dev.close()


def test_two_rdm_budget_ignores_the_previous_buffer():
    """A second afq_bp_observables frees the M^4 buffer of the first before it checks the budget."""
    model, h1e, Lv, rng = build(64, 4, 3, 3)
    dev = make_device(model, 2)
    dev.bp_configure(2)
    for _ in range(3):
        dev.bp_observables(two_rdm=True, ekt=True, h1=h1e)
    dev.close()
