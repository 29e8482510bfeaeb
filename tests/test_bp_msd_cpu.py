"""The back-propagation window of a multi-determinant trial without a GPU: the fp64 restatement (tests/bp_msd_ref.py)
against the extended-precision one, the identities the specification implies (they are repeated on the device in
tests/test_gpu_bp_msd.py), the genuine reference's per-determinant pieces (tests/golden/bp_msd.npz) and the façade."""
import types

import numpy
import pytest

from oracle import afqmc_ref as ref
from pauxy_amd import systems
from pauxy_amd.estimators.back_propagation import BackPropagation
from pauxy_amd.estimators.itcf import ITCF
from tests import bp_msd_ref as R, itcf_ref, itcf_ref_ext as X


def case(M, K, na, nb, nd, nw, n, seed, hermitian=False):
    """A Generic model (symmetric real or Hermitian complex vectors), nd complex determinants, nw walkers' window
    starts, fields [n, nw, K] and weights."""
    rng = numpy.random.RandomState(seed)
    h = rng.normal(size=(M, M))
    h1e = 0.5 * (h + h.T) - 2.0 * numpy.eye(M)
    A = rng.normal(size=(K, M, M)) * (0.3 / numpy.sqrt(M))
    if hermitian:
        A = A + 1j * rng.normal(size=(K, M, M)) * (0.3 / numpy.sqrt(M))
        Lv = 0.5 * (A + A.conj().transpose(0, 2, 1))
    else:
        Lv = 0.5 * (A + A.transpose(0, 2, 1))
    hs_pot = numpy.ascontiguousarray(Lv.reshape(K, M * M).T)
    dt = 0.01
    e, v = numpy.linalg.eigh(h1e)
    BT2 = numpy.array([(v * numpy.exp(-0.5 * dt * e)).dot(v.T)] * 2).astype(complex)
    base = numpy.hstack([v[:, :na], v[:, :nb]]).astype(complex)
    ne = na + nb
    dets = numpy.array([base + 0.1 * (rng.rand(M, ne) + 1j * rng.rand(M, ne)) for _ in range(nd)])
    coeffs = (rng.normal(size=nd) + 1j * rng.normal(size=nd)) * 0.5 + 1.0
    phi_old = numpy.array([base + 0.1 * (rng.rand(M, ne) + 1j * rng.rand(M, ne)) for _ in range(nw)])
    xs = rng.normal(size=(n, nw, K)) + 0.2j * rng.normal(size=(n, nw, K))
    wt = rng.rand(nw) + 0.5
    energy = (numpy.array([h1e, h1e]).astype(complex), 0.1, hs_pot)
    return types.SimpleNamespace(M=M, K=K, na=na, nb=nb, hs_pot=hs_pot, BT2=BT2, dt=dt, dets=dets, coeffs=coeffs,
                                 phi_old=phi_old, xs=xs, wt=wt, energy=energy, h1e=h1e)


def windows64(c, nstblz, dets=None, coeffs=None, energy=False):
    dets = c.dets if dets is None else dets
    coeffs = c.coeffs if coeffs is None else coeffs
    return [R.window64(R.b64(c.hs_pot, c.BT2, c.xs[:, w], c.dt), c.phi_old[w], dets, coeffs, c.na, nstblz,
                       c.energy if energy else None) for w in range(len(c.wt))]


def rel(a, b):
    return float(numpy.max(numpy.abs(numpy.asarray(a) - numpy.asarray(b))) / max(1.0, float(numpy.max(numpy.abs(b)))))


CASES = [("M=12 3+3 ndet=3 nstblz=1", dict(M=12, K=9, na=3, nb=3, nd=3, nw=3, n=4, seed=3), 1),
         ("M=16 5+3 ndet=2 nstblz=2 (H)", dict(M=16, K=10, na=5, nb=3, nd=2, nw=2, n=5, seed=4, hermitian=True), 2),
         ("M=24 6+5 ndet=4 nstblz>=n", dict(M=24, K=12, na=6, nb=5, nd=4, nw=2, n=3, seed=5), 7)]


@pytest.mark.parametrize("name,kw,nstblz", CASES, ids=[c[0].replace(' ', '_') for c in CASES])
def test_fp64_restatement_against_the_extended_one(name, kw, nstblz):
    """err_ref of the rule: the fp64 restatement's distance from the extended one is a few roundings per element, so
    bound(err_ref) is of order 1e-13 for these shapes."""
    c = case(**kw)
    wins = windows64(c, nstblz, energy=True)
    E64, den64, G64 = R.sums64(wins, c.wt)
    w64 = numpy.array([w['w'] / w['S'] for w in wins])
    Ex, denx, Gx, wx = R.sums_ext(c.hs_pot, c.BT2, c.dt, c.xs, c.phi_old, c.dets, c.coeffs, c.na, nstblz, c.wt, c.energy)
    errs = R.slice_errors(R.slices(E64, G64, w64), R.slices(Ex, Gx, wx))
    err_ref = float(numpy.max(errs))
    print("BPMSD-REF | %s | err_ref %.2e | bound %.2e | per slice %s" % (name, err_ref, X.bound(err_ref),
                                                                        ' '.join('%.1e' % e for e in errs)))
    assert abs(complex(denx) - den64) < 1e-14 * abs(den64)
    assert err_ref <= 1e-13
    assert X.bound(err_ref) <= 1e-11


def test_one_determinant_is_the_oracle_window():
    """ndet = 1: the window of oracle/afqmc_ref.py: bp_update, which the GPU tests hold the single-determinant device
    path to (real fields: the oracle's histories are what the walk records; energies included)."""
    c = case(M=12, K=9, na=3, nb=3, nd=1, nw=3, n=4, seed=6)
    c.xs = c.xs.real.astype(complex)
    for nstblz in (1, 2, 9):
        model = types.SimpleNamespace(M=c.M, na=c.na, kind='generic', psi=c.dets[0], hs_pot=c.hs_pot, BH1=c.BT2,
                                      dt=c.dt, H1=c.energy[0], ecore=c.energy[1])
        walkers = [dict(bp=dict(configs=c.xs[:, w].copy(), step=len(c.xs)), phi_old=c.phi_old[w], phi=c.phi_old[w],
                        weight=c.wt[w]) for w in range(len(c.wt))]
        est = numpy.zeros(4 + 2 * c.M * c.M, dtype=complex)
        ref.bp_update(model, walkers, nstblz, est, eval_energy=True, reset=False)
        E, den, G = R.sums64(windows64(c, nstblz, coeffs=numpy.array([0.3 - 0.8j]), energy=True), c.wt)
        assert rel(G.ravel(), est[4:]) < 1e-12 and rel(E, est[:3]) < 1e-12 and abs(den - est[3]) < 1e-13


@pytest.mark.parametrize("nstblz", [1, 2, 9])
def test_copies_of_one_determinant_are_the_single_determinant_window(nstblz):
    c = case(M=12, K=9, na=3, nb=3, nd=1, nw=3, n=5, seed=7)
    one = windows64(c, nstblz, energy=True)
    three = windows64(c, nstblz, dets=numpy.array([c.dets[0]] * 3), coeffs=numpy.array([0.7 + 0.2j, -0.3 + 0.5j, 0.1j]),
                      energy=True)
    for a, b in zip(one, three):
        assert rel(b['G'], a['G']) < 1e-12 and rel(b['E'], a['E']) < 1e-12
        assert rel(b['w'] / b['S'], numpy.array([0.7 - 0.2j, -0.3 - 0.5j, -0.1j]) / (0.4 - 0.8j)) < 1e-12


def unitary(n, rng):
    q, _ = numpy.linalg.qr(rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n)))
    return q


@pytest.mark.parametrize("nstblz", [1, 2, 9])
def test_rotating_a_determinant_changes_nothing(nstblz):
    """|D U> = det U |D> for U unitary and block-diagonal in spin: D_d -> D_d U_d with c_d -> c_d / det U_d is the
    same many-body trial, so every w_d, G_bp and the energies are unchanged."""
    c = case(M=12, K=9, na=4, nb=3, nd=3, nw=2, n=5, seed=8)
    rng = numpy.random.RandomState(1)
    dets, coeffs = c.dets.copy(), c.coeffs.copy()
    for d in range(3):
        Ua, Ub = unitary(c.na, rng), unitary(c.nb, rng)
        dets[d] = numpy.hstack([c.dets[d][:, :c.na].dot(Ua), c.dets[d][:, c.na:].dot(Ub)])
        coeffs[d] = c.coeffs[d] / (numpy.linalg.det(Ua) * numpy.linalg.det(Ub))
    for a, b in zip(windows64(c, nstblz, energy=True), windows64(c, nstblz, dets=dets, coeffs=coeffs, energy=True)):
        assert rel(b['w'] / b['S'], a['w'] / a['S']) < 1e-11
        assert rel(b['G'], a['G']) < 1e-11 and rel(b['E'], a['E']) < 1e-11


def test_backward_and_forward_agree_on_the_overlap():
    """nstblz >= nbp (log r_d = 0): sum_d w_d = sum_d conj(c_d) det(D_d^H phi_n), phi_n = B(x_n) .. B(x_1) phi_old."""
    c = case(M=12, K=9, na=3, nb=3, nd=3, nw=3, n=4, seed=9)
    for w, win in enumerate(windows64(c, 9)):
        assert numpy.all(win['logr'] == 0)
        Bs = R.b64(c.hs_pot, c.BT2, c.xs[:, w], c.dt)
        phi = [c.phi_old[w][:, :c.na], c.phi_old[w][:, c.na:]]
        for B in Bs:
            phi = [B[s].dot(phi[s]) for s in range(2)]
        fwd = sum(numpy.conj(c.coeffs[d]) * numpy.linalg.det(c.dets[d][:, :c.na].conj().T.dot(phi[0]))
                  * numpy.linalg.det(c.dets[d][:, c.na:].conj().T.dot(phi[1])) for d in range(3))
        assert abs(win['S'] - fwd) < 1e-12 * abs(fwd)


def test_norms_of_the_reorthogonalisation_matter():
    """Dropping log r_d (what a single determinant may do) changes the weights of a multi-determinant window: the
    re-orthogonalised window with its norms equals the one that is never re-orthogonalised, without them it does not."""
    c = case(M=12, K=9, na=3, nb=3, nd=3, nw=2, n=5, seed=10)
    for a, b in zip(windows64(c, 1), windows64(c, 9)):
        assert rel(a['w'] / a['S'], b['w'] / b['S']) < 1e-11 and rel(a['G'], b['G']) < 1e-11
        assert numpy.ptp(a['logr']) > 1e-3


def test_restatement_reproduces_the_reference_pieces(golden):
    """tests/golden/bp_msd.npz: the genuine back_propagate_generic on every determinant over genuine-format histories
    (nstblz > nbp), composed with the genuine gab; per-op tolerance of the golden tests (rel 1e-10)."""
    d = golden('bp_msd.npz')
    na = int(d['nelec'][0])
    nstblz = int(d['nstblz'])
    for w in range(len(d['fields'])):
        Bs = R.b64(d['hs_pot'], d['BT2'], d['fields'][w], float(d['dt']))
        win = R.window64(Bs, d['phi_old'][w], d['dets'], d['coeffs'], na, nstblz)
        want_w = numpy.conj(d['coeffs']) * d['ovlp'][w]
        assert numpy.all(win['logr'] == 0)
        assert rel(win['w'], want_w) < 1e-10 and rel(win['Gd'], d['G'][w]) < 1e-10
        G = numpy.tensordot(want_w, d['G'][w], axes=(0, 0)) / numpy.sum(want_w)
        assert rel(win['G'], G) < 1e-10
        for i in range(len(d['dets'])):
            Q, lr = R.backward64(Bs, d['dets'][i], na, nstblz)
            assert rel(Q, d['bp'][w, i]) < 1e-10


# ---------------------------------------------------------------------------------------------------- façade
def generic(M=5, K=6):
    rng = numpy.random.RandomState(1)
    h = rng.normal(size=(M, M))
    A = rng.normal(size=(K, M, M))
    Lv = 0.5 * (A + A.transpose(0, 2, 1))
    return systems.Generic((2, 2), numpy.array([h + h.T, h + h.T]), numpy.ascontiguousarray(Lv.reshape(K, M * M).T),
                           ecore=0.0)


QMC = types.SimpleNamespace(dt=0.005, nstblz=5)


def make(bp, ndets, system=None):
    trial = types.SimpleNamespace(ndets=ndets)
    return BackPropagation(dict(bp, tau_bp=0.025), True, None, QMC, system or generic(), trial, complex, None)


def test_facade_accepts_a_multi_determinant_trial():
    one, three = make({'evaluate_energy': True}, 1), make({'evaluate_energy': True}, 3)
    assert three.nmax == one.nmax == 5 and sorted(three.__dict__) == sorted(one.__dict__)
    assert three.estimates.size == one.estimates.size == 3 + 1 + 2 * 25
    assert numpy.array_equal(three.splits, one.splits) and three.header == one.header
    for k in ('two_rdm', 'fock_1p', 'fock_1h'):
        assert k not in three.__dict__
    split = make({'nsplit': 5, 'restore_weights': 'full', 'init_walker': True}, 3)
    assert list(split.splits) == [1, 2, 3, 4, 5] and split.restore_weights == 'full' and split.init_walker


class Comm(object):
    rank = 0

    def Reduce(self, a, b, op=None):
        b[:] = a


def test_facade_slicing_is_the_single_determinant_one():
    out = []
    for nd in (1, 3):
        est = make({'evaluate_energy': True}, nd)
        est.estimates[:] = numpy.arange(est.estimates.size) + 0.5j
        est.accumulated = True
        est.buff_ix = 5
        est.print_step(Comm(), 1, 0)
        out.append((est.denominator[0], est.energies[0], est.one_rdm[0]))
    assert all(numpy.array_equal(a, b) for a, b in zip(*out))


def test_facade_refusals():
    with pytest.raises(NotImplementedError):
        make({'two_rdm': True}, 3)
    with pytest.raises(NotImplementedError):
        make({'evaluate_ekt': True}, 3)
    with pytest.raises(NotImplementedError):
        make({}, 3, systems.Hubbard(4, 4, 7, 7, 4.0))
    make({'two_rdm': True, 'evaluate_ekt': True}, 1)
    s = generic()
    qmc = types.SimpleNamespace(dt=0.005, nstblz=5, nsteps=10)
    with pytest.raises(NotImplementedError):
        ITCF({'tau_max': 0.02}, qmc, types.SimpleNamespace(ndets=3), False, None, s, complex, None)
