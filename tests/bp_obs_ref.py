"""numpy restatement of the back-propagated two-body RDM and EKT Fock matrices
(estimators/back_propagation.py:168-175, estimators/ekt.py:10-73 of the reference), written from the formulas:

  two_rdm[p,r,q,s] = S[p,r] S[q,s] - sum_s G_s[p,s] G_s[q,r],   S = G_a + G_b
  X_s[x] = sum_ik L_x[i,k] G_s[i,k],   C_s = sum_x X_s[x] L_x^T
  F1p = (2I - G_a^T - G_b^T) h1 + 2 (C_a + C_b) - 2 G_a^T C_b - G_a^T C_a - G_b^T C_b
        + sum_x [ -L_x (G_a + G_b)^T L_x^T + G_a^T L_x G_a^T L_x^T + G_b^T L_x G_b^T L_x^T ]
  F1h = -(G_a + G_b) h1^T - 2 G_a C_b^T - G_a C_a^T - G_b C_b^T + sum_x [ G_a L_x^T G_a L_x + G_a L_x^T G_b L_x ]

Plain transposes throughout, no conjugates.  L has the shape [nL, M, M]."""
import numpy


def two_rdm(Ga, Gb):
    S = Ga + Gb
    return (numpy.einsum('pr,qs->prqs', S, S) - numpy.einsum('ps,qr->prqs', Ga, Ga)
            - numpy.einsum('ps,qr->prqs', Gb, Gb))


def _coulomb(L, G):
    X = numpy.einsum('xik,ik->x', L, G)
    return numpy.einsum('x,xki->ik', X, L)          # sum_x X[x] L_x^T


def fock_1p(h1, L, Ga, Gb):
    M = h1.shape[0]
    Ca, Cb = _coulomb(L, Ga), _coulomb(L, Gb)
    R = Ga + Gb
    F = (2.0 * numpy.eye(M) - Ga.T - Gb.T) @ h1 + 2.0 * (Ca + Cb) - 2.0 * Ga.T @ Cb - Ga.T @ Ca - Gb.T @ Cb
    LT = L.transpose(0, 2, 1)
    F = F - numpy.einsum('xij,jk,xkl->il', L, R.T, LT, optimize=True)
    for G in (Ga, Gb):
        T = numpy.einsum('ij,xjk->xik', G.T, L)          # G^T L_x
        F = F + numpy.einsum('xij,jk,xkl->il', T, G.T, LT, optimize=True)
    return F


def fock_1h(h1, L, Ga, Gb):
    Ca, Cb = _coulomb(L, Ga), _coulomb(L, Gb)
    F = -(Ga + Gb) @ h1.T - 2.0 * Ga @ Cb.T - Ga @ Ca.T - Gb @ Cb.T
    LT = L.transpose(0, 2, 1)
    U = numpy.einsum('ij,xjk->xik', Ga, LT)              # G_a L_x^T
    for G in (Ga, Gb):
        F = F + numpy.einsum('xij,jk,xkl->il', U, G, L, optimize=True)
    return F


def window(h1, L, Gs, wts, two=True, ekt=True):
    """sum_w wt_w (two_rdm, fock_1p, fock_1h) of Green's functions Gs[w, 2, M, M] (None where not asked for)."""
    out = [None, None, None]
    for G, wt in zip(Gs, wts):
        if two:
            t = wt * two_rdm(G[0], G[1])
            out[0] = t if out[0] is None else out[0] + t
        if ekt:
            a, b = wt * fock_1p(h1, L, G[0], G[1]), wt * fock_1h(h1, L, G[0], G[1])
            out[1] = a if out[1] is None else out[1] + a
            out[2] = b if out[2] is None else out[2] + b
    return out
