"""numpy restatement of the imaginary-time single-particle Green's function (ITCF) of one window, written from the
specification in DESIGN.md (row 8f-3) rather than from the reference's estimators/itcf.py, whose composed output is
not sound:

  B_t = BT2_s E(x_t) BT2_s;  E = sum_{k<=6} V^k / k!, V = i sqrt(dt) sum_n x_n L_n  (Generic)
                             E = diag(auxf[x_t, s])                                 (discrete Hubbard fields)
  psi_R(0) = phi (window start), psi_R(t+1) = B_t psi_R(t), re-orthogonalised after step t when t != 0, t % nstblz == 0
  psi_L(n) = psi_T, psi_L(t) = B_t^H psi_L(t+1), re-orthogonalised after the i-th step from the end, i != 0, i % nstblz == 0
  P(t) = gab(psi_L(t), psi_R(t)) per spin, G^> = I - P, G^< = P
  stable:   Ggr(0) = I - P(0), Gls(0) = P(0); Ggr(t+1) = B_t (I - P(t)) Ggr(t), Gls(t+1) = Gls(t) P(t) B_t^-1
  unstable: Ggr(t+1) = B_t Ggr(t), Gls(t+1) = Gls(t) B_t^-1
  spgf[t, s, 0] = sum_w wfac_w Re Ggr_s(t), spgf[t, s, 1] = sum_w wfac_w Re Gls_s(t)
"""
import numpy


def gab(A, B):
    """estimators/greens_function.py:5: B (A^H B)^-1 A^H."""
    return B.dot(numpy.linalg.inv(A.conj().T.dot(B)).dot(A.conj().T))


def reortho(A):
    """utils/linalg.py reortho: the Q of A's economic QR with a positive diagonal of R."""
    Q, R = numpy.linalg.qr(A)
    signs = numpy.sign(numpy.diag(R).real)
    signs[signs == 0] = 1.0
    return Q * signs[None, :]


def exponentiate_matrix(V, order=6):
    """utils/linalg.py:163-170."""
    T = V.copy()
    E = numpy.identity(V.shape[0], dtype=V.dtype)
    for n in range(1, order + 1):
        E = E + T
        T = V.dot(T) / (n + 1)
    return E


def b_generic(hs_pot, BT2, x, dt):
    """propagation/generic.py:181-207: [B_up, B_down] of the fields x."""
    M = BT2.shape[-1]
    V = 1j * dt ** 0.5 * numpy.asarray(hs_pot).dot(x).reshape(M, M)
    E = exponentiate_matrix(V)
    return numpy.array([BT2[0].dot(E).dot(BT2[0]), BT2[1].dot(E).dot(BT2[1])])


def b_hirsch(BT2, x, dt, U):
    """propagation/hubbard.py:568-600: [B_up, B_down] of the discrete fields x (0 / 1 per site)."""
    gamma = numpy.arccosh(numpy.exp(0.5 * dt * U))
    auxf = numpy.array([[numpy.exp(gamma), numpy.exp(-gamma)], [numpy.exp(-gamma), numpy.exp(gamma)]])
    x = numpy.asarray(x).real.astype(int)
    return numpy.array([BT2[s].dot(auxf[x, s][:, None] * BT2[s]) for s in range(2)])


def spins(psi, na):
    return [psi[:, :na], psi[:, na:]]


def back_propagate(Bs, psi_T, na, nstblz):
    """psi_L(t) = B_t^H psi_L(t+1) from psi_L(n) = psi_T, per spin ([up, down] for t = 0 .. n-1), re-orthogonalised
    after the i-th step from the end when i != 0 and i % nstblz == 0 (propagation/generic.py:253-290)."""
    n = len(Bs)
    psiL = [None] * n
    left = [p.copy() for p in spins(psi_T, na)]
    for i in range(n):
        t = n - 1 - i
        left = [Bs[t, s].conj().T.dot(left[s]) for s in range(2)]
        if i != 0 and i % nstblz == 0:
            left = [reortho(p) for p in left]
        psiL[t] = left
    return psiL


def window(Bs, phi, psi_T, na, nmax, nstblz, stable=True):
    """(Ggr, Gls) [nmax + 1, 2, M, M] of one walker: Bs [n, 2, M, M] the window's matrices, phi its determinant at the
    window start, psi_T the trial."""
    n = len(Bs)
    M = Bs.shape[-1]
    I = numpy.identity(M)
    psiL = back_propagate(Bs, psi_T, na, nstblz)
    right = [p.copy() for p in spins(phi, na)]
    Ggr = numpy.zeros((nmax + 1, 2, M, M), dtype=complex)
    Gls = numpy.zeros((nmax + 1, 2, M, M), dtype=complex)
    P = [gab(psiL[0][s], right[s]) for s in range(2)]
    for s in range(2):
        Ggr[0, s] = I - P[s]
        Gls[0, s] = P[s]
    for t in range(nmax):
        Binv = [numpy.linalg.inv(Bs[t, s]) for s in range(2)]
        if stable:
            P = [gab(psiL[t][s], right[s]) for s in range(2)]
            for s in range(2):
                Ggr[t + 1, s] = Bs[t, s].dot(I - P[s]).dot(Ggr[t, s])
                Gls[t + 1, s] = Gls[t, s].dot(P[s]).dot(Binv[s])
            right = [Bs[t, s].dot(right[s]) for s in range(2)]
            if t != 0 and t % nstblz == 0:
                right = [reortho(p) for p in right]
        else:
            for s in range(2):
                Ggr[t + 1, s] = Bs[t, s].dot(Ggr[t, s])
                Gls[t + 1, s] = Gls[t, s].dot(Binv[s])
    return Ggr, Gls


def accumulate(windows, wfac):
    """spgf [nmax + 1, 2, 2, M, M] = sum_w wfac_w (Re Ggr_w, Re Gls_w); walkers with wfac 0 are skipped."""
    out = None
    for win, wt in zip(windows, wfac):
        if wt == 0:
            continue
        Ggr, Gls = win
        term = wt * numpy.stack([Ggr.real, Gls.real], axis=2)
        out = term if out is None else out + term
    return out


def select(spgf, mode):
    """The written form of spgf [.., 2, 2, M, M]: 'full', 'diagonal' or the elements of a list of (i, j) pairs."""
    if mode == 'full':
        return spgf
    if mode == 'diagonal':
        return numpy.diagonal(spgf, axis1=-2, axis2=-1)
    ij = numpy.array(mode, dtype=int).reshape(-1, 2)
    return spgf[..., ij[:, 0], ij[:, 1]]
