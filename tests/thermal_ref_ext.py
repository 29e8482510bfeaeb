"""The finite-temperature path of tests/thermal_ref.py in extended precision (numpy.longdouble: on x86-64 a 64-bit
mantissa, eps 1.1e-19).  numpy.linalg and scipy do not take the type, so the column-pivoted Householder QR and the
inverse (Gauss-Jordan with partial pivoting, tests/itcf_ref_ext.py) are the module's own; both work on stacks
[nb, M, M], every matrix with its own pivots, so that a population costs one pass of numpy loops.

The path logic is thermal_ref.Path run with this module's number type and routines (KitExt).

The rule the device is tested under is the project's (tests/itcf_ref_ext.py): MARGIN = 100, FLOOR = 1e-15.
  err_ref = max |fp64 restatement - this module| for a compared G, on the same fields
  the device's G must lie within bound(err_ref) = 100 max(err_ref, 1e-15) of this module's
  weights: within M x (slices so far) x that bound, relative (every site multiplies the weight by a quantity
           linear in G_ii)
  energies and nav (linear in G): within the bound x (||H1||_1 + U M)"""
import numpy

from tests import thermal_ref
from tests.itcf_ref_ext import FLOOR, LD, MARGIN, bound  # noqa: F401  (the rule, re-exported)


def ext(a):
    return numpy.asarray(a, dtype=LD)


def inv(A):
    """A^-1 of a real stack [..., n, n]: Gauss-Jordan on [A | I], the pivot of a column its largest remaining element."""
    A = ext(A)
    n = A.shape[-1]
    lead = A.shape[:-2]
    nb = int(numpy.prod(lead, dtype=int))
    W = numpy.concatenate([A.reshape((nb, n, n)), numpy.broadcast_to(numpy.eye(n, dtype=LD), (nb, n, n))], axis=2)
    b = numpy.arange(nb)
    for c in range(n):
        p = c + numpy.argmax(numpy.abs(W[:, c:, c]), axis=1)
        top = W[b, c].copy()
        W[b, c] = W[b, p]
        W[b, p] = top
        W[:, c] = W[:, c] / W[:, c, c][:, None]
        f = W[:, :, c].copy()
        f[:, c] = 0
        W = W - f[:, :, None] * W[:, c][:, None, :]
    return W[:, :, n:].reshape(lead + (n, n))


def qrcp(A):
    """A[b] P_b = Q_b R_b for a stack [nb, n, n] -> (Q^T, R, perm): Householder reflections, the pivot of step j the
    remaining column of the largest norm over the rows j.., norms recomputed at every step."""
    W = ext(A).copy()
    nb, n, _ = W.shape
    Qt = numpy.broadcast_to(numpy.eye(n, dtype=LD), (nb, n, n)).copy()
    perm = numpy.broadcast_to(numpy.arange(n), (nb, n)).copy()
    b = numpy.arange(nb)
    for j in range(n):
        nrm2 = numpy.sum(W[:, j:, j:] ** 2, axis=1)
        p = j + numpy.argmax(nrm2, axis=1)
        cj = W[b, :, j].copy()
        W[b, :, j] = W[b, :, p]
        W[b, :, p] = cj
        pj = perm[b, j].copy()
        perm[b, j] = perm[b, p]
        perm[b, p] = pj
        x = W[:, j:, j].copy()
        nrm = numpy.sqrt(numpy.sum(x ** 2, axis=1))
        x0 = x[:, 0]
        alpha = numpy.where(x0 >= 0, -nrm, nrm)
        v = x / (x0 - alpha)[:, None]
        v[:, 0] = 1
        tau = (alpha - x0) / alpha
        sw = numpy.einsum('bi,bic->bc', v, W[:, j:, j:])
        W[:, j:, j:] -= (tau[:, None] * v)[:, :, None] * sw[:, None, :]
        sq = numpy.einsum('bi,bic->bc', v, Qt[:, j:, :])
        Qt[:, j:, :] -= (tau[:, None] * v)[:, :, None] * sq[:, None, :]
        W[:, j, j] = alpha
        W[:, j + 1:, j] = 0
    return Qt, W, perm


def graded(R, perm):
    """(D, D^-1 R P^T) of an upper-triangular stack and its column permutations."""
    n = R.shape[-1]
    D = numpy.diagonal(R, axis1=-2, axis2=-1).copy()
    T = numpy.zeros_like(R)
    numpy.put_along_axis(T, numpy.broadcast_to(perm[:, None, :], R.shape), numpy.triu(R) / D[:, :, None], axis=2)
    assert T.shape[-1] == n
    return D, T


def strat_greens(bins):
    """bins: list of [nb, M, M] stacks in chain order -> G [nb, M, M]."""
    Qt, R, perm = qrcp(bins[0])
    D, T = graded(R, perm)
    for B in bins[1:]:
        C = (ext(B) @ numpy.swapaxes(Qt, -1, -2)) * D[:, None, :]
        Qt, R, perm = qrcp(C)
        D, t = graded(R, perm)
        T = t @ T
    Db, Ds = thermal_ref.split_d(D)
    Tinv = inv(T)
    right = Db[:, :, None] * Qt
    C = right @ Tinv
    i = numpy.arange(C.shape[-1])
    C[:, i, i] += Ds
    return Tinv @ inv(C) @ right


class KitExt(object):
    dtype = LD
    strat_greens = staticmethod(strat_greens)
    inv = staticmethod(inv)


def path(BT, BH1, auxf, L, stack_size, nstblz, nw, BT_inv=None):
    """thermal_ref.Path in extended precision.  BT_inv: the inverse the device is given (fp64), so that both wrap G
    with the same matrices; None inverts BT here."""
    return thermal_ref.Path(ext(BT), ext(BH1), ext(auxf), L, stack_size, nstblz, nw, kit=KitExt, BT_inv=BT_inv)


def gerr(got, want):
    """max |got - want| over a stack of Green's functions, evaluated in extended precision."""
    return float(numpy.max(numpy.abs(ext(got) - ext(want))))
