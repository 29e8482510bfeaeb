"""The finite-temperature UEG path of tests/thermal_ueg_ref.py in extended precision (numpy.clongdouble: on x86-64 a
64-bit mantissa, eps 1.1e-19).  numpy.linalg and scipy do not take the type, so the column-pivoted QR with complex
Householder reflectors, the determinant (LU with partial pivoting) and the inverse (Gauss-Jordan, tests/itcf_ref_ext.py)
are the module's own; all work on stacks [nb, M, M], every matrix with its own pivots.

The path logic is thermal_ueg_ref.Path run with this module's number types and routines (KitExt).

The rule the device is tested under is the project's (tests/itcf_ref_ext.py): MARGIN = 100, FLOOR = 1e-15.
  err_ref = max |fp64 restatement - this module| for a compared quantity, on the same inputs, on the scale
            max(1, max |quantity|)
  the device must lie within bound(err_ref) = 100 max(err_ref, 1e-15) of this module's on the same scale
  determinants: the same rule relative to |det|"""
import numpy

from tests import thermal_ueg_ref
from tests.itcf_ref_ext import CLD, FLOOR, LD, MARGIN, bound, inv  # noqa: F401  (the rule, re-exported)


def ext(a):
    return numpy.asarray(a, dtype=CLD)


def qrcp(A):
    """A[b] P_b = Q_b R_b for a complex stack [nb, n, n] -> (Q^H, R, perm): reflections H = I - tau v v^H with
    H x = -(x_0 / |x_0|) ||x|| e_0, the pivot of step j the remaining column of the largest norm over the rows j.."""
    W = ext(A).copy()
    nb, n, _ = W.shape
    Qh = numpy.broadcast_to(numpy.eye(n, dtype=CLD), (nb, n, n)).copy()
    perm = numpy.broadcast_to(numpy.arange(n), (nb, n)).copy()
    b = numpy.arange(nb)
    for j in range(n):
        nrm2 = numpy.sum(numpy.abs(W[:, j:, j:]) ** 2, axis=1)
        p = j + numpy.argmax(nrm2, axis=1)
        cj = W[b, :, j].copy()
        W[b, :, j] = W[b, :, p]
        W[b, :, p] = cj
        pj = perm[b, j].copy()
        perm[b, j] = perm[b, p]
        perm[b, p] = pj
        x = W[:, j:, j].copy()
        nrm = numpy.sqrt(numpy.sum(numpy.abs(x) ** 2, axis=1))
        x0 = x[:, 0]
        a0 = numpy.abs(x0)
        ph = numpy.where(a0 > 0, x0 / numpy.where(a0 > 0, a0, 1), 1)
        alpha = -ph * nrm
        v = x / (x0 - alpha)[:, None]
        v[:, 0] = 1
        tau = (nrm + a0) / nrm
        sw = numpy.einsum('bi,bic->bc', numpy.conj(v), W[:, j:, j:])
        W[:, j:, j:] -= (tau[:, None] * v)[:, :, None] * sw[:, None, :]
        sq = numpy.einsum('bi,bic->bc', numpy.conj(v), Qh[:, j:, :])
        Qh[:, j:, :] -= (tau[:, None] * v)[:, :, None] * sq[:, None, :]
        W[:, j, j] = alpha
        W[:, j + 1:, j] = 0
    return Qh, W, perm


def graded(R, perm):
    """(D, D^-1 R P^T) of an upper-triangular stack and its column permutations."""
    D = numpy.diagonal(R, axis1=-2, axis2=-1).copy()
    T = numpy.zeros_like(R)
    numpy.put_along_axis(T, numpy.broadcast_to(perm[:, None, :], R.shape), numpy.triu(R) / D[:, :, None], axis=2)
    return D, T


def strat_greens(bins):
    """bins: list of [nb, M, M] complex stacks in chain order -> G [nb, M, M]."""
    Qh, R, perm = qrcp(bins[0])
    D, T = graded(R, perm)
    for B in bins[1:]:
        C = (ext(B) @ numpy.conj(numpy.swapaxes(Qh, -1, -2))) * D[:, None, :]
        Qh, R, perm = qrcp(C)
        D, t = graded(R, perm)
        T = t @ T
    Db, Ds = thermal_ueg_ref.split_d(D)
    Tinv = inv(T)
    right = Db[:, :, None] * Qh
    C = right @ Tinv
    i = numpy.arange(C.shape[-1])
    C[:, i, i] += Ds
    return Tinv @ inv(C) @ right


def det(A):
    """det of a complex stack [..., n, n]: the product of the pivots of an LU with partial pivoting."""
    A = ext(A)
    n = A.shape[-1]
    lead = A.shape[:-2]
    W = A.reshape((-1, n, n)).copy()
    nb = W.shape[0]
    b = numpy.arange(nb)
    d = numpy.ones(nb, dtype=CLD)
    for c in range(n):
        p = c + numpy.argmax(numpy.abs(W[:, c:, c]), axis=1)
        top = W[b, c].copy()
        W[b, c] = W[b, p]
        W[b, p] = top
        d = numpy.where(p != c, -d, d) * W[:, c, c]
        f = W[:, c + 1:, c] / W[:, c, c][:, None]
        W[:, c + 1:, :] -= f[:, :, None] * W[:, c][:, None, :]
    return d.reshape(lead)


class KitExt(object):
    dtype = CLD
    rtype = LD
    strat_greens = staticmethod(strat_greens)
    det = staticmethod(det)


def path(ops, BTdiag, BTinvdiag, BH1diag, dt, L, stack_size, nw, mf_shift=None, fb_bound=1.0):
    """thermal_ueg_ref.Path in extended precision; ops: thermal_ueg_ref.Operators(system, KitExt).  BT_inv is the
    inverse the device is given (fp64), so that both build left_k from the same numbers."""
    return thermal_ueg_ref.Path(ops, BTdiag, BTinvdiag, BH1diag, dt, L, stack_size, nw, kit=KitExt, mf_shift=mf_shift,
                                fb_bound=fb_bound)


def gerr(got, want, scale=None):
    """max |got - want| on the scale max(1, max |want|) (or the scale given), evaluated in extended precision."""
    want = ext(want)
    s = max(1.0, float(numpy.max(numpy.abs(want)))) if scale is None else scale
    return float(numpy.max(numpy.abs(ext(got) - want))) / s


def rerr(got, want):
    """max |got / want - 1|: determinants and weights."""
    return float(numpy.max(numpy.abs(ext(got) / ext(want) - 1)))
