"""The imaginary-time Green's function without a GPU: the numpy restatement (tests/itcf_ref.py) against its own
identities, the estimator's options, output shapes and refusals."""
import numpy
import pytest
import scipy.linalg

from pauxy_amd import systems, trial as trial_mod
from pauxy_amd.estimators.handler import Estimators
from pauxy_amd.estimators.itcf import ITCF
from pauxy_amd.qmc.options import QMCOpts
from tests import itcf_ref


def generic_case(M=10, K=12, na=4, nb=3, seed=0, dt=0.01, cplx=None):
    rng = numpy.random.RandomState(seed)
    A = rng.normal(size=(K, M, M)) * (0.3 / numpy.sqrt(M))
    if cplx == 'hermitian':
        A = A + 1j * rng.normal(size=(K, M, M)) * (0.3 / numpy.sqrt(M))
        Lv = 0.5 * (A + A.conj().transpose(0, 2, 1))
    elif cplx == 'general':
        Lv = A + 1j * rng.normal(size=(K, M, M)) * (0.3 / numpy.sqrt(M))
    else:
        Lv = 0.5 * (A + A.transpose(0, 2, 1))
    hs = numpy.ascontiguousarray(Lv.reshape(K, M * M).T)
    h = rng.normal(size=(M, M))
    h = 0.5 * (h + h.T)
    e, v = numpy.linalg.eigh(h)
    psi = numpy.hstack([v[:, :na], v[:, :nb]]).astype(complex) + 0.05 * rng.rand(M, na + nb)
    s = systems.Generic((na, nb), numpy.array([h, h]), hs, ecore=0.0)
    BT2 = numpy.array([scipy.linalg.expm(-0.5 * dt * h)] * 2)
    return s, psi, BT2, rng


def generic_window(n, nmax, nstblz, stable, seed=0, M=10, na=4, nb=3, cplx=None):
    s, psi, BT2, rng = generic_case(M=M, na=na, nb=nb, seed=seed, cplx=cplx)
    K = s.hs_pot.shape[1]
    Bs = numpy.array([itcf_ref.b_generic(s.hs_pot, BT2, rng.normal(size=K) + 0.2j * rng.normal(size=K), 0.01)
                      for _ in range(n)])
    phi = psi + 0.1 * (rng.rand(*psi.shape) + 1j * rng.rand(*psi.shape))
    return itcf_ref.window(Bs, phi, psi, na, nmax, nstblz, stable)


def hirsch_window(n, nmax, nstblz, stable, nx=4, na=7, nb=5, seed=1, dt=0.05, U=4.0):
    s = systems.Hubbard(nx, nx, na, nb, U)
    M = nx * nx
    T = numpy.asarray(s.T)
    BT2 = numpy.array([scipy.linalg.expm(-0.5 * dt * T[i]) for i in range(2)])
    rng = numpy.random.RandomState(seed)
    e, v = numpy.linalg.eigh(T[0])
    psi = numpy.hstack([v[:, :na], v[:, :nb]]).astype(complex)
    Bs = numpy.array([itcf_ref.b_hirsch(BT2, rng.randint(0, 2, size=M), dt, U) for _ in range(n)])
    phi = psi + 0.05 * rng.rand(M, na + nb)
    return itcf_ref.window(Bs, phi, psi, na, nmax, nstblz, stable)


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("n,nmax,nstblz", [(10, 10, 20), (10, 10, 3), (14, 10, 4), (12, 10, 1)])
def test_stable_equals_unstable_generic(n, nmax, nstblz):
    """(I - P(t+1)) B_t = B_t (I - P(t)) and P idempotent: both chains give the same functions, re-orthogonalised
    inside the window or not."""
    a = generic_window(n, nmax, nstblz, True)
    b = generic_window(n, nmax, nstblz, False)
    for x, y in zip(a, b):
        assert numpy.abs(x - y).max() <= 1e-10 * max(1.0, numpy.abs(y).max())


@pytest.mark.parametrize("n,nmax,nstblz", [(10, 10, 3), (13, 10, 5)])
def test_stable_equals_unstable_hirsch(n, nmax, nstblz):
    a = hirsch_window(n, nmax, nstblz, True)
    b = hirsch_window(n, nmax, nstblz, False)
    for x, y in zip(a, b):
        assert numpy.abs(x - y).max() <= 1e-10 * max(1.0, numpy.abs(y).max())


def test_stable_equals_unstable_hermitian_vectors():
    a = generic_window(10, 8, 3, True, cplx='hermitian')
    b = generic_window(10, 8, 3, False, cplx='hermitian')
    for x, y in zip(a, b):
        assert numpy.abs(x - y).max() <= 1e-10 * max(1.0, numpy.abs(y).max())


@pytest.mark.parametrize("which", ['generic', 'hirsch'])
def test_equal_time_functions(which):
    """Ggr(0) + Gls(0) = I and tr Ggr_s(0) = M - N_s, tr Gls_s(0) = N_s."""
    if which == 'generic':
        Ggr, Gls = generic_window(8, 6, 3, True)
        M, ns = 10, (4, 3)
    else:
        Ggr, Gls = hirsch_window(8, 6, 3, True)
        M, ns = 16, (7, 5)
    for s in range(2):
        assert numpy.abs(Ggr[0, s] + Gls[0, s] - numpy.eye(M)).max() < 1e-12
        assert abs(numpy.trace(Ggr[0, s]) - (M - ns[s])) < 1e-10
        assert abs(numpy.trace(Gls[0, s]) - ns[s]) < 1e-10


def test_propagator_matrices_follow_their_definitions():
    """B = BT2 E BT2 with the order-6 Taylor E (close to expm(V)), and the discrete B = BT2 diag(auxf[x, s]) BT2."""
    s, psi, BT2, rng = generic_case()
    K = s.hs_pot.shape[1]
    x = rng.normal(size=K)
    B = itcf_ref.b_generic(s.hs_pot, BT2, x, 0.01)
    V = 1j * 0.1 * s.hs_pot.dot(x).reshape(10, 10)
    for sp in range(2):
        assert numpy.abs(B[sp] - BT2[sp].dot(scipy.linalg.expm(V)).dot(BT2[sp])).max() < 1e-8
    BT2h = numpy.array([scipy.linalg.expm(-0.025 * numpy.eye(4))] * 2)
    f = itcf_ref.b_hirsch(BT2h, numpy.array([0, 1, 1, 0]), 0.05, 4.0)
    g = numpy.arccosh(numpy.exp(0.1))
    assert numpy.allclose(numpy.diag(f[0]) / numpy.exp(-0.05), numpy.exp([g, -g, -g, g]))
    assert numpy.allclose(numpy.diag(f[1]) / numpy.exp(-0.05), numpy.exp([-g, g, g, -g]))


def test_accumulate_skips_zero_weights():
    Ggr = numpy.ones((2, 2, 3, 3)) * (1 + 1j)
    nan = numpy.full((2, 2, 3, 3), numpy.nan)
    out = itcf_ref.accumulate([(Ggr, 2 * Ggr), (nan, nan), (Ggr, Ggr)], [0.5 + 0.5j, 0.0, 2.0])
    assert numpy.allclose(out[:, :, 0], 2.5 + 0.5j) and numpy.allclose(out[:, :, 1], 3.0 + 1.0j)


# ---------------------------------------------------------------- the estimator
def make(opts, system=None, trial=None, dt=0.01, nstblz=5, **kw):
    if system is None:
        system, psi, BT2, rng = generic_case()
        trial = trial_mod.SingleDetTrial(system, psi)
    qmc = QMCOpts({'timestep': dt, 'num_steps': 10, 'blocks': 1, 'stabilise_freq': nstblz}, system)
    return ITCF(opts, qmc, trial, False, None, system, complex, None, **kw), qmc, system, trial


def test_options_and_attributes():
    est, qmc, s, t = make({'tau_max': 0.05, 'tau_eqlb': 0.02})
    assert (est.nmax, est.ntau, est.neqlb, est.nprop_tot) == (5, 5, 2, 7)
    assert est.stable is True and est.restore_weights is True and est.mode == 'full'
    assert est.spgf_shape == (6, 2, 2, 10, 10) and est.spgf.shape == est.spgf_shape and est.denom == 0
    est.spgf[:] = 1.0
    est.denom = 3.0
    est.zero()
    assert not est.spgf.any() and est.denom == 0
    est, *_ = make({'tau_max': 0.03, 'stable': False, 'restore_weights': False})
    assert (est.nmax, est.neqlb, est.nprop_tot, est.stable, est.restore_weights) == (3, 0, 3, False, False)


@pytest.mark.parametrize("mode,shape", [('full', (4, 2, 2, 10, 10)), ('diagonal', (4, 2, 2, 10)),
                                        ([[0, 1], [2, 2], [9, 3]], (4, 2, 2, 3))])
def test_written_shapes(mode, shape):
    est, *_ = make({'tau_max': 0.03, 'mode': mode})
    g = numpy.random.RandomState(0).rand(4, 2, 2, 10, 10)
    out = est.written(g)
    assert out.shape == shape
    assert numpy.array_equal(out, itcf_ref.select(g, mode))
    if mode == 'diagonal':
        assert out[1, 0, 1, 7] == g[1, 0, 1, 7, 7]
    elif mode != 'full':
        assert out[2, 1, 0, 2] == g[2, 1, 0, 9, 3]


def test_update_waits_for_the_window_end():
    est, qmc, s, t = make({'tau_max': 0.03, 'tau_eqlb': 0.01})

    class NoDevice(object):
        def __getattr__(self, name):
            raise AssertionError("the walkers were touched at step %r" % name)
    for step in (0, 1, 2, 3, 5, 7):
        est.update(s, qmc, t, NoDevice(), step)


def test_refusals():
    with pytest.raises(NotImplementedError, match='UEG'):
        ueg = type('UEG', (), {'name': 'UEG', 'nbasis': 19})()
        make({'tau_max': 0.02}, system=ueg, trial=None)
    hub = systems.Hubbard(2, 2, 1, 1, 4.0)
    ht = type('T', (), {'ndets': 1})()
    with pytest.raises(NotImplementedError, match='continuous Hubbard'):
        make({'tau_max': 0.02, 'restore_weights': False}, system=hub, trial=ht, discrete=False)
    with pytest.raises(NotImplementedError, match='restore_weights'):
        make({'tau_max': 0.02}, system=hub, trial=ht, discrete=True)
    est, *_ = make({'tau_max': 0.02, 'restore_weights': False}, system=hub, trial=ht, discrete=True)
    assert est.nmax == 2
    s, psi, BT2, rng = generic_case()
    with pytest.raises(NotImplementedError, match='multi-determinant'):
        make({'tau_max': 0.02}, system=s, trial=type('T', (), {'ndets': 3})())
    t = trial_mod.SingleDetTrial(s, psi)
    with pytest.raises(NotImplementedError, match='free projection'):
        make({'tau_max': 0.02}, system=s, trial=t, free_projection=True)
    with pytest.raises(NotImplementedError, match='kspace'):
        make({'tau_max': 0.02, 'kspace': True}, system=s, trial=t)
    with pytest.raises(NotImplementedError, match='stack_size'):
        make({'tau_max': 0.02, 'stack_size': 2}, system=s, trial=t)
    with pytest.raises(ValueError):
        make({'tau_max': 0.001}, system=s, trial=t)
    sg, psig, _, _ = generic_case(cplx='general')
    with pytest.raises(NotImplementedError, match='non-Hermitian'):
        make({'tau_max': 0.02}, system=sg, trial=trial_mod.SingleDetTrial(sg, psig))
    sh, psih, _, _ = generic_case(cplx='hermitian')
    make({'tau_max': 0.02}, system=sh, trial=trial_mod.SingleDetTrial(sh, psih))
    big = type('G', (), {'name': 'Generic', 'nbasis': 129, 'hs_pot': numpy.zeros((4, 2))})()
    with pytest.raises(NotImplementedError, match='128'):
        make({'tau_max': 0.02}, system=big, trial=ht)


def test_handler_builds_the_estimator_and_refuses_two_windows():
    s, psi, BT2, rng = generic_case()
    t = trial_mod.SingleDetTrial(s, psi)
    qmc = QMCOpts({'timestep': 0.01, 'num_steps': 10, 'blocks': 1}, s)
    est = Estimators({'itcf': {'tau_max': 0.04, 'tau_eqlb': 0.02}, 'write_file': False}, True, qmc, s, t, None)
    assert isinstance(est.estimators['itcf'], ITCF)
    assert est.nprop_tot == 6 and est.nbp is None and est.calc_itcf
    with pytest.raises(NotImplementedError, match='back_propagation'):
        Estimators({'itcf': {'tau_max': 0.04}, 'back_propagated': {'tau_bp': 0.02}, 'write_file': False}, True, qmc,
                   s, t, None)
    plain = Estimators({'write_file': False}, True, qmc, s, t, None)
    assert plain.nprop_tot is None and not plain.calc_itcf and 'itcf' not in plain.estimators
