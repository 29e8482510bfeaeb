"""The extended-precision restatement of the ITCF (tests/itcf_ref_ext.py): its own linear algebra by residuals, its
building blocks against the recorded reference values, its windows against the fp64 restatement, and the reason it
exists: two plausible wrong windows that a tolerance of 1e-8 passes are outside the bound the device is held to."""
import numpy
import pytest

from tests import itcf_ref, itcf_ref_ext as X
from tests.test_itcf_golden_cpu import close


def synthetic(M, K, na, nb, n, seed=3, dt=0.01, hermitian=False):
    """A generic_model-like system without the library: vectors [M*M, K], BT2, trial, one walker, n steps of fields."""
    rng = numpy.random.RandomState(seed)
    h = rng.normal(size=(M, M))
    h1e = 0.5 * (h + h.T) - 2.0 * numpy.eye(M)
    A = rng.normal(size=(K, M, M)) * (0.3 / numpy.sqrt(M))
    if hermitian:
        A = A + 1j * rng.normal(size=(K, M, M)) * (0.3 / numpy.sqrt(M))
    Lv = 0.5 * (A + A.conj().transpose(0, 2, 1))
    hs = numpy.ascontiguousarray(Lv.reshape(K, M * M).T)
    e, v = numpy.linalg.eigh(h1e)
    BT2 = numpy.array([(v * numpy.exp(-0.5 * dt * e)) @ v.T] * 2).astype(complex)
    psi = numpy.zeros((M, na + nb), dtype=complex)
    psi[:, :na] = v[:, :na]
    psi[:, na:] = v[:, :nb]
    psi = psi + 0.05 * (rng.rand(M, na + nb) + 1j * rng.rand(M, na + nb))
    phi = psi + 0.1 * (rng.rand(M, na + nb) + 1j * rng.rand(M, na + nb))
    xs = rng.normal(size=(n, K)) + 0.05j * rng.normal(size=(n, K))
    return hs, BT2, psi, phi, xs, dt


def spgf(win):
    return numpy.stack([win[0].real, win[1].real], axis=2)


def worst(got, want):
    return float(numpy.max(X.slice_errors(spgf(got), spgf(want))))


def test_longdouble_is_extended():
    assert numpy.finfo(X.LD).nmant >= 63 and numpy.finfo(X.LD).eps < 2e-19
    assert X.inv(numpy.eye(3)).dtype == X.CLD


@pytest.mark.parametrize("n", [0, 1, 2, 7, 33])
def test_inverse_by_its_residual(n):
    rng = numpy.random.RandomState(n)
    A = rng.normal(size=(3, n, n)) + 1j * rng.normal(size=(3, n, n))
    if n > 1:
        A[1, 0, 0] = 0.0                                 # a zero on the diagonal: the pivot search has to move off it
    Ai = X.inv(A)
    assert Ai.shape == A.shape and Ai.dtype == X.CLD
    I = numpy.eye(n, dtype=X.CLD)
    for k in range(3):
        cond = float(numpy.linalg.cond(A[k])) if n else 1.0
        assert float(numpy.max(numpy.abs(X.ext(A[k]) @ Ai[k] - I), initial=0)) <= 1e-17 * n * cond
        assert float(numpy.max(numpy.abs(Ai[k] @ X.ext(A[k]) - I), initial=0)) <= 1e-17 * n * cond
        if n:
            close(Ai[k].astype(complex), numpy.linalg.inv(A[k]), 1e-13 * cond)


@pytest.mark.parametrize("M,n", [(5, 0), (5, 1), (16, 5), (40, 40), (64, 13)])
def test_reortho_by_its_residual(M, n):
    rng = numpy.random.RandomState(M + n)
    A = rng.normal(size=(2, M, n)) + 1j * rng.normal(size=(2, M, n))
    Q = X.reortho(A)
    assert Q.shape == A.shape and Q.dtype == X.CLD
    for k in range(2):
        assert float(numpy.max(numpy.abs(X.dagger(Q[k]) @ Q[k] - numpy.eye(n)), initial=0)) <= 1e-17 * max(n, 1)
        R = X.dagger(Q[k]) @ X.ext(A[k])                 # upper triangular with a positive diagonal, and A = Q R
        assert float(numpy.max(numpy.abs(numpy.tril(R, -1)), initial=0)) <= 1e-16 * M
        assert numpy.all(numpy.diag(R).real > 0)
        assert float(numpy.max(numpy.abs(Q[k] @ R - A[k]), initial=0)) <= 1e-16 * M
        want = itcf_ref.reortho(A[k])
        for j in range(n):
            close(Q[k][:, j].astype(complex), want[:, j], 1e-12)


@pytest.mark.parametrize("M,n", [(6, 0), (6, 1), (16, 5), (16, 16), (48, 17)])
def test_gab_is_the_oblique_projector(M, n):
    rng = numpy.random.RandomState(M * n + 1)
    A = rng.normal(size=(M, n)) + 1j * rng.normal(size=(M, n))
    B = A + 0.3 * (rng.normal(size=(M, n)) + 1j * rng.normal(size=(M, n)))
    P = X.gab(A, B)
    assert P.shape == (M, M)
    tol = 1e-16 * M * (float(numpy.linalg.cond(A.conj().T @ B)) if n else 1.0)
    assert float(numpy.max(numpy.abs(P @ P - P), initial=0)) <= tol                      # idempotent
    assert float(numpy.max(numpy.abs(P @ X.ext(B) - B), initial=0)) <= tol               # the identity on span(B)
    assert float(numpy.max(numpy.abs(X.dagger(X.ext(A)) @ P - X.dagger(X.ext(A))), initial=0)) <= tol
    assert abs(complex(numpy.trace(P)) - n) <= tol * M
    if n == M:
        assert float(numpy.max(numpy.abs(P - numpy.eye(M)))) <= tol                      # a filled band: P = I
    if n:
        close(P.astype(complex), itcf_ref.gab(A, B), 1e-12)


def test_blocks_against_the_recorded_reference(golden):
    """The tolerance of test_itcf_golden_cpu.py (1e-12)."""
    d = golden('itcf_blocks.npz')
    dt = float(d['g_dt'])
    for x, B in zip(d['g_fields'], d['g_B']):
        close(X.b_generic(d['g_hs_pot'], d['g_BT2'], x, dt).astype(complex), B)
    close(X.b_generic(d['g_hs_pot'], d['g_BT2'], d['g_fields'], dt).astype(complex), d['g_B'].swapaxes(0, 1))   # stacked
    for x, B in zip(d['h_fields'], d['h_B']):
        close(X.b_hirsch(d['h_BT2'], x, float(d['h_dt']), float(d['h_U'])).astype(complex), B)
    close(X.gab(d['gab_A'], d['gab_B']).astype(complex), d['gab'])
    close(X.reortho(d['reortho_in']).astype(complex), d['reortho_Q'])
    Bs = numpy.array([X.b_generic(d['g_hs_pot'], d['g_BT2'], x, dt) for x in d['g_fields']])
    psiL = X.back_propagate(Bs, d['g_bp_phi'], int(d['g_nelec'][0]), int(d['g_bp_nstblz']))
    n = len(Bs)
    assert len(d['g_bp_store']) == n
    for i in range(n):
        close(numpy.hstack(psiL[n - 1 - i]).astype(complex), d['g_bp_store'][i])


@pytest.mark.parametrize("stable", [True, False])
@pytest.mark.parametrize("M,K,na,nb,nmax,neqlb,nstblz,hermitian", [
    (16, 24, 5, 3, 7, 2, 3, False), (16, 20, 5, 3, 5, 2, 3, True), (12, 10, 4, 0, 4, 1, 2, False),
    (8, 6, 8, 7, 3, 0, 1, False), (33, 20, 9, 9, 6, 1, 2, False)])
def test_generic_windows_against_the_fp64_restatement(M, K, na, nb, nmax, neqlb, nstblz, hermitian, stable):
    hs, BT2, psi, phi, xs, dt = synthetic(M, K, na, nb, nmax + neqlb, hermitian=hermitian)
    B64 = numpy.array([itcf_ref.b_generic(hs, BT2, x, dt) for x in xs])
    Bx = numpy.array([X.b_generic(hs, BT2, x, dt) for x in xs])
    assert float(numpy.max(numpy.abs(Bx - B64))) <= 1e-14
    g64 = itcf_ref.window(B64, phi, psi, na, nmax, nstblz, stable)
    gx = X.window(Bx, phi, psi, na, nmax, nstblz, stable)
    assert gx[0].shape == g64[0].shape and gx[0].dtype == X.CLD
    for a, b in zip(g64, gx):
        assert float(numpy.max(numpy.abs(a - b))) <= 1e-13 * max(1.0, float(numpy.max(numpy.abs(b))))
    assert worst(g64, gx) <= 1e-13


def test_a_stack_of_walkers_is_the_walkers_one_by_one():
    M, K, na, nb, nmax, neqlb, nstblz = 10, 8, 3, 2, 3, 1, 2
    hs, BT2, psi, phi, xs, dt = synthetic(M, K, na, nb, nmax + neqlb)
    rng = numpy.random.RandomState(9)
    phis = numpy.array([phi + 0.05 * rng.rand(M, na + nb) for _ in range(3)])
    xw = rng.normal(size=(nmax + neqlb, 3, K))
    Bs = numpy.array([X.b_generic(hs, BT2, xw[t], dt) for t in range(nmax + neqlb)])      # [n, 2, 3, M, M]
    wfac = numpy.array([0.5, 1.25, 2.0])
    for stable in (True, False):
        all_ = X.window(Bs, phis, psi, na, nmax, nstblz, stable)
        one = [X.window(Bs[:, :, w], phis[w], psi, na, nmax, nstblz, stable) for w in range(3)]
        for w in range(3):
            assert float(numpy.max(numpy.abs(all_[0][:, :, w] - one[w][0]))) <= 1e-17
            assert float(numpy.max(numpy.abs(all_[1][:, :, w] - one[w][1]))) <= 1e-17
        assert float(numpy.max(numpy.abs(X.accumulate_stack(all_, wfac) - X.accumulate(one, wfac)))) <= 1e-17


@pytest.mark.parametrize("stable", [True, False])
@pytest.mark.parametrize("nx,ny,na,nb,nmax,neqlb,nstblz", [(3, 3, 5, 4, 4, 1, 2), (4, 2, 4, 4, 3, 0, 1)])
def test_hirsch_windows_against_the_fp64_restatement(nx, ny, na, nb, nmax, neqlb, nstblz, stable):
    M, U, dt = nx * ny, 4.0, 0.05
    rng = numpy.random.RandomState(5)
    T = numpy.zeros((M, M))
    for i in range(M):
        for j in ((i + 1) % M, (i + nx) % M):
            if i != j:
                T[i, j] = T[j, i] = -1.0
    e, v = numpy.linalg.eigh(T)
    BT2 = numpy.array([(v * numpy.exp(-0.5 * dt * e)) @ v.T] * 2).astype(complex)
    psi = numpy.hstack([v[:, :na], v[:, :nb]]).astype(complex)
    phi = psi + 0.05 * rng.rand(M, na + nb)
    fields = rng.randint(0, 2, size=(nmax + neqlb, M))
    B64 = numpy.array([itcf_ref.b_hirsch(BT2, f, dt, U) for f in fields])
    Bx = numpy.array([X.b_hirsch(BT2, f, dt, U) for f in fields])
    assert float(numpy.max(numpy.abs(Bx - B64))) <= 1e-14
    assert worst(itcf_ref.window(B64, phi, psi, na, nmax, nstblz, stable),
                 X.window(Bx, phi, psi, na, nmax, nstblz, stable)) <= 1e-13


@pytest.mark.parametrize("stable", [True, False])
def test_mutations_a_tolerance_of_1e8_passes_are_outside_the_bound(monkeypatch, stable):
    """M = 16, 5+3, nmax 7, neqlb 2: B^-1 taken as BT2^-1 E(-V) BT2^-1 (the Taylor series of -V, not the inverse of the
    truncated series of V), and a Taylor series of order 5, both applied to the fp64 restatement.  Only the wrong
    inverse slips under the old tolerance of 1e-8 (1.2e-9 of the largest element of the window); order 5 is 1.2e-7 off
    and shows the berth of the bound: neither is within it, by more than two orders."""
    M, K, na, nb, nmax, neqlb, nstblz = 16, 24, 5, 3, 7, 2, 3
    hs, BT2, psi, phi, xs, dt = synthetic(M, K, na, nb, nmax + neqlb)
    truth = X.window(numpy.array([X.b_generic(hs, BT2, x, dt) for x in xs]), phi, psi, na, nmax, nstblz, stable)
    B64 = numpy.array([itcf_ref.b_generic(hs, BT2, x, dt) for x in xs])
    good = itcf_ref.window(B64, phi, psi, na, nmax, nstblz, stable)
    err_ref = worst(good, truth)
    limit = X.bound(err_ref)
    assert err_ref <= 1e-14

    def b5(x):
        E = itcf_ref.exponentiate_matrix(1j * dt ** 0.5 * hs.dot(x).reshape(M, M), 5)
        return numpy.array([BT2[0] @ E @ BT2[0], BT2[1] @ E @ BT2[1]])
    order5 = itcf_ref.window(numpy.array([b5(x) for x in xs]), phi, psi, na, nmax, nstblz, stable)

    wrong, real_inv = {}, numpy.linalg.inv
    BT2i = real_inv(BT2[0])
    for t, x in enumerate(xs):
        Em = itcf_ref.exponentiate_matrix(-1j * dt ** 0.5 * hs.dot(x).reshape(M, M))
        for s in range(2):
            wrong[B64[t, s].tobytes()] = BT2i @ Em @ BT2i
    monkeypatch.setattr(numpy.linalg, 'inv', lambda A: wrong[A.tobytes()] if A.tobytes() in wrong else real_inv(A))
    taylor_inverse = itcf_ref.window(B64, phi, psi, na, nmax, nstblz, stable)
    monkeypatch.undo()

    for name, mutant in (('order 5', order5), ('Taylor series of -V as the inverse', taylor_inverse)):
        err = worst(mutant, truth)
        whole = max(float(numpy.max(numpy.abs(a - b))) / max(1.0, float(numpy.max(numpy.abs(b))))
                    for a, b in zip(mutant, truth))
        print("%s, stable=%s: err_ref %.2e, bound %.2e, mutant %.2e (whole-array %.2e)" % (name, stable, err_ref, limit,
                                                                                            err, whole))
        assert err > limit, (name, err, limit)
        assert err > 100 * limit, (name, err, limit)             # and by a wide berth
    assert worst(taylor_inverse, truth) <= 1e-8                   # the tolerance this replaces let that one through
