"""The restatement of tests/itcf_ref.py in extended precision (numpy.longdouble / numpy.clongdouble: on x86-64 a 64-bit
mantissa, eps 1.1e-19), written from the same specification (the docstring of itcf_ref.py):

  B_t = BT2_s E(x_t) BT2_s;  E = sum_{k<=6} V^k / k!, V = i sqrt(dt) sum_n x_n L_n  (Generic)
                             E = diag(auxf[x_t, s])                                 (discrete Hubbard fields)
  psi_R(0) = phi (window start), psi_R(t+1) = B_t psi_R(t), re-orthogonalised after step t when t != 0, t % nstblz == 0
  psi_L(n) = psi_T, psi_L(t) = B_t^H psi_L(t+1), re-orthogonalised after the i-th step from the end, i != 0, i % nstblz == 0
  P(t) = gab(psi_L(t), psi_R(t)) per spin, G^> = I - P, G^< = P
  stable:   Ggr(0) = I - P(0), Gls(0) = P(0); Ggr(t+1) = B_t (I - P(t)) Ggr(t), Gls(t+1) = Gls(t) P(t) B_t^-1
  unstable: Ggr(t+1) = B_t Ggr(t), Gls(t+1) = Gls(t) B_t^-1

numpy.linalg does not take these types, so the inverse (Gauss-Jordan with partial pivoting) and the
re-orthogonalisation (Gram-Schmidt applied twice; the diagonal of R is a norm, hence positive) are the module's own.
Every function takes stacks: leading axes in front of the matrix axes are walkers, so a whole population costs one pass
of numpy loops rather than one per walker.

It also holds the rule the device is tested under (slice_errors, bound): see their docstrings."""
import numpy

LD, CLD = numpy.longdouble, numpy.clongdouble
assert numpy.finfo(LD).nmant > 52 and numpy.finfo(LD).eps < 2e-19, \
    "numpy.longdouble is not wider than 64 bits here: no extended-precision reference"

MARGIN = 100.0          # over the fp64 restatement's own distance from this module: see bound()
FLOOR = 1e-15           # about the smallest err_ref of a non-trivial shape


def ext(a):
    return numpy.asarray(a, dtype=CLD)


def dagger(A):
    return numpy.conj(numpy.swapaxes(A, -1, -2))


def inv(A):
    """A^-1 of a stack [..., n, n]: Gauss-Jordan on [A | I], the pivot of a column its largest remaining element."""
    A = ext(A)
    n = A.shape[-1]
    lead = A.shape[:-2]
    nb = int(numpy.prod(lead, dtype=int))
    W = numpy.concatenate([A.reshape((nb, n, n)), numpy.broadcast_to(numpy.eye(n, dtype=CLD), (nb, n, n))], axis=2)
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


def reortho(A):
    """The Q of A = Q R with a positive diagonal of R, of a stack [..., M, n]: every column is projected off its
    predecessors twice and then normalised."""
    Q = ext(A).copy()
    for j in range(Q.shape[-1]):
        for _ in range(2):
            c = dagger(Q[..., :j]) @ Q[..., j:j + 1]
            Q[..., j:j + 1] = Q[..., j:j + 1] - Q[..., :j] @ c
        nrm = numpy.sqrt(numpy.sum(numpy.abs(Q[..., j]) ** 2, axis=-1))
        Q[..., j] = Q[..., j] / nrm[..., None]
    return Q


def gab(A, B):
    """B (A^H B)^-1 A^H."""
    A, B = ext(A), ext(B)
    return B @ inv(dagger(A) @ B) @ dagger(A)


def exponentiate_matrix(V, order=6):
    T = V.copy()
    E = numpy.broadcast_to(numpy.eye(V.shape[-1], dtype=CLD), V.shape).copy()
    for n in range(1, order + 1):
        E = E + T
        T = (V @ T) / LD(n + 1)
    return E


def b_generic(hs_pot, BT2, x, dt):
    """[B_up, B_down] (axis 0) of the fields x [..., K]: [2, ..., M, M]."""
    BT2 = ext(BT2)
    M = BT2.shape[-1]
    x = ext(x)
    V = (1j * numpy.sqrt(LD(dt))) * (x @ ext(hs_pot).T).reshape(x.shape[:-1] + (M, M))
    E = exponentiate_matrix(V)
    return numpy.array([BT2[0] @ E @ BT2[0], BT2[1] @ E @ BT2[1]])


def b_hirsch(BT2, x, dt, U):
    """[B_up, B_down] of the discrete fields x [..., M] (0 / 1 per site); auxf is the spin decomposition's."""
    BT2 = ext(BT2)
    gamma = numpy.arccosh(numpy.exp(LD(0.5) * LD(dt) * LD(U)))
    auxf = numpy.array([[numpy.exp(gamma), numpy.exp(-gamma)], [numpy.exp(-gamma), numpy.exp(gamma)]], dtype=LD)
    x = numpy.asarray(x).real.astype(int)
    return numpy.array([BT2[s] @ (auxf[x, s][..., :, None] * BT2[s]) for s in range(2)])


def spins(psi, na):
    psi = ext(psi)
    return [psi[..., :na], psi[..., na:]]


def back_propagate(Bs, psi_T, na, nstblz):
    """psi_L(t) per spin ([up, down] for t = 0 .. n-1) of Bs [n, 2, ..., M, M]."""
    n = len(Bs)
    psiL = [None] * n
    left = spins(psi_T, na)
    for i in range(n):
        t = n - 1 - i
        left = [dagger(Bs[t][s]) @ left[s] for s in range(2)]
        if i != 0 and i % nstblz == 0:
            left = [reortho(p) for p in left]
        psiL[t] = left
    return psiL


def window(Bs, phi, psi_T, na, nmax, nstblz, stable=True):
    """(Ggr, Gls) [nmax + 1, 2, ..., M, M]: Bs [n, 2, ..., M, M] the window's matrices, phi [..., M, ne] the
    determinants at the window start, psi_T [M, ne] the trial."""
    M = Bs[0][0].shape[-1]
    I = numpy.eye(M, dtype=CLD)
    psiL = back_propagate(Bs, psi_T, na, nstblz)
    right = spins(phi, na)
    P = [gab(psiL[0][s], right[s]) for s in range(2)]
    Ggr = [[I - P[s] for s in range(2)]]
    Gls = [[P[s] for s in range(2)]]
    for t in range(nmax):
        Binv = [inv(Bs[t][s]) for s in range(2)]
        if stable:
            P = [gab(psiL[t][s], right[s]) for s in range(2)]
            Ggr.append([Bs[t][s] @ (I - P[s]) @ Ggr[t][s] for s in range(2)])
            Gls.append([Gls[t][s] @ P[s] @ Binv[s] for s in range(2)])
            right = [Bs[t][s] @ right[s] for s in range(2)]
            if t != 0 and t % nstblz == 0:
                right = [reortho(p) for p in right]
        else:
            Ggr.append([Bs[t][s] @ Ggr[t][s] for s in range(2)])
            Gls.append([Gls[t][s] @ Binv[s] for s in range(2)])
    return numpy.array(Ggr), numpy.array(Gls)


def accumulate(windows, wfac):
    """spgf [nmax + 1, 2, 2, M, M] = sum_w wfac_w (Re Ggr_w, Re Gls_w); walkers with wfac 0 are skipped."""
    out = None
    for win, wt in zip(windows, wfac):
        if wt == 0:
            continue
        Ggr, Gls = win
        term = CLD(wt) * numpy.stack([Ggr.real, Gls.real], axis=2)
        out = term if out is None else out + term
    return out


def accumulate_stack(win, wfac):
    """accumulate() of a window whose single walker axis (axis 2 of Ggr / Gls) holds the walkers of wfac (none 0)."""
    Ggr, Gls = win
    wt = ext(wfac)[None, None, :, None, None]
    return numpy.stack([numpy.sum(wt * Ggr.real, axis=2), numpy.sum(wt * Gls.real, axis=2)], axis=2)


def window_sums(kind, model, fields, phi, psi_T, na, nmax, nstblz, stable, wfac):
    """accumulate_stack() of the windows of a stack of walkers from their recorded fields [n, nw, ...]: kind 'generic'
    with model = (hs_pot, BT2, dt), or 'hirsch' with model = (BT2, dt, U).  A plain function of plain arrays, so that a
    population can be dealt over worker processes."""
    if kind == 'generic':
        hs_pot, BT2, dt = model
        hs_pot = ext(hs_pot)
        Bs = [b_generic(hs_pot, BT2, x, dt) for x in fields]
    else:
        BT2, dt, U = model
        Bs = [b_hirsch(BT2, x, dt, U) for x in fields]
    return accumulate_stack(window(Bs, phi, psi_T, na, nmax, nstblz, stable), wfac)


# ---- the rule the device's window sums are tested under
def slice_errors(got, want):
    """Per slice (tau, spin, greater / lesser) of spgf-shaped arrays [nmax + 1, 2, 2, ...]: max |got - want| over the
    slice / max(1, max |want| over the slice), evaluated in extended precision."""
    got, want = ext(got), ext(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    flat = (got.shape[0], 2, 2, -1)
    diff = numpy.max(numpy.abs(got - want).reshape(flat), axis=-1)
    scale = numpy.maximum(LD(1), numpy.max(numpy.abs(want).reshape(flat), axis=-1))
    return (diff / scale).astype(float)


def bound(err_ref):
    """What the device may differ by, per slice and on the slice's scale, from the extended restatement's sums:
    MARGIN x max(err_ref, FLOOR), err_ref the largest slice error of the fp64 restatement of the same case against the
    extended one.  MARGIN is a margin over a measurement: two decimal orders over what a LAPACK-based fp64 evaluation
    of the same chain loses.  Gauss-Jordan / Gram-Schmidt run in fp64 land within 1.0-1.1 x of LAPACK's error, so the
    evaluation order alone is worth little; the rest is for the device summing up to a thousand walkers serially per
    element and for a backward pass through production kernels whose complex products are bounded norm-wise, not
    element-wise.  The floor keeps a lucky case from demanding less than a few roundings per element."""
    return MARGIN * max(float(err_ref), FLOOR)
