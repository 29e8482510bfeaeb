"""Restatements of the back-propagation window of a multi-determinant trial |psi_T> = sum_d c_d |D_d> (DESIGN.md row
8f-2, include/afqmc_hip.h: afq_bp_update_msd), written from that specification; the reference has no such window (its
BackPropagation fails on ndets > 1).  Per walker, over its recorded shifted fields x_1 .. x_n (forward order), the walker
at the window's start phi_old and its weight wt in the window:

  D_d^bp = B(x_1)^H .. B(x_n)^H D_d, applied from x_n down, B(x) = BT2_s E(x) BT2_s, E the order-6 Taylor exponential
           of V = i sqrt(dt) sum_k x_k L_k; re-orthogonalised per spin after the i-th step from the end when i != 0 and
           i % nstblz == 0: D = Q R with diag R > 0, D <- Q, log r_d += log det R_alpha + log det R_beta
  w_d    = conj(c_d) exp(log r_d - max_d' log r_d') det(Q_d,alpha^H phi_old,alpha) det(Q_d,beta^H phi_old,beta)
           (zero or not finite: zero); S = sum_d w_d (zero or not finite: the walker does not count)
  G_d    = gab(Q_d, phi_old)^T per spin, G_bp = sum_d w_d G_d / S, E = sum_d w_d E[G_d] / S (full-G Cholesky energy)
  sums   = (sum_w wt_w E_w, sum_w wt_w, sum_w wt_w G_bp[w])

window64: plain fp64 numpy (LAPACK's QR, inverse and determinant), one walker.  window_ext: numpy.longdouble with the
helpers of tests/itcf_ref_ext.py, a stack of walkers.  compare(): the rule of that module (bound) on one window."""
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy

from tests import itcf_ref, itcf_ref_ext as X

LD, CLD = X.LD, X.CLD


# ---------------------------------------------------------------------------------------------------- fp64
def energy64(H1, ecore, G, chol):
    """estimators/generic.py:398-434: (E, E1b, E2b) of G [2, M, M] with chol [M*M, K]."""
    M = G.shape[-1]
    K = chol.shape[-1]
    e1b = numpy.sum(H1[0] * G[0]) + numpy.sum(H1[1] * G[1])
    Xa, Xb = chol.T.dot(G[0].ravel()), chol.T.dot(G[1].ravel())
    ecoul = Xa.dot(Xa) + Xb.dot(Xb) + 2 * Xa.dot(Xb)
    cv = chol.reshape(M, M, K)
    exx = 0.0
    for g in G:
        T = numpy.tensordot(g, cv, axes=((0), (0)))
        exx = exx + numpy.tensordot(T, T, axes=((0, 1, 2), (1, 0, 2)))
    e2b = 0.5 * (ecoul - exx)
    return numpy.array([e1b + e2b + ecore, e1b + ecore, e2b])


def qr_pos(A):
    """A = Q R with a positive diagonal of R -> (Q, log det R)."""
    Q, R = numpy.linalg.qr(A)
    d = numpy.diag(R)
    ph = d / numpy.abs(d)
    return Q * ph[None, :], float(numpy.sum(numpy.log(numpy.abs(d))))


def backward64(Bs, D, na, nstblz):
    """(Q [M, ne], log r) of one determinant through Bs [n, 2, M, M]."""
    left = [D[:, :na].astype(complex), D[:, na:].astype(complex)]
    logr = 0.0
    n = len(Bs)
    for i in range(n):
        t = n - 1 - i
        left = [Bs[t][s].conj().T.dot(left[s]) for s in range(2)]
        if i != 0 and i % nstblz == 0:
            for s in range(2):
                if left[s].shape[1]:
                    left[s], lr = qr_pos(left[s])
                    logr += lr
    return numpy.hstack(left), logr


def combine(coeffs, logr, ovlp):
    """w_d (un-normalised) and S; a w_d that is not finite counts as zero."""
    logr = numpy.asarray(logr)
    with numpy.errstate(all='ignore'):
        w = numpy.conj(coeffs) * numpy.exp(logr - numpy.max(logr)) * ovlp
    w = numpy.where(numpy.isfinite(w), w, 0)
    return w, numpy.sum(w)


def window64(Bs, phi_old, dets, coeffs, na, nstblz, energy=None):
    """One walker: dict(w [nd] un-normalised, S, logr, Gd [nd, 2, M, M], G [2, M, M], E [3] or None).  Bs [n, 2, M, M];
    energy = (H1, ecore, chol)."""
    nd = len(dets)
    Gd, ov, logr, Ed = [], [], [], []
    for d in range(nd):
        Q, lr = backward64(Bs, dets[d], na, nstblz)
        o = 1.0
        g = []
        for sl in (slice(0, na), slice(na, None)):
            A, B = Q[:, sl], phi_old[:, sl]
            o = o * numpy.linalg.det(A.conj().T.dot(B))
            g.append(itcf_ref.gab(A, B).T)
        Gd.append(numpy.array(g))
        ov.append(o)
        logr.append(lr)
        if energy is not None:
            Ed.append(energy64(energy[0], energy[1], Gd[-1], energy[2]))
    w, S = combine(numpy.asarray(coeffs), logr, numpy.array(ov))
    Gd = numpy.array(Gd)
    G = numpy.tensordot(w, Gd, axes=(0, 0)) / S
    E = numpy.tensordot(w, numpy.array(Ed), axes=(0, 0)) / S if energy is not None else None
    return dict(w=w, S=S, logr=numpy.array(logr), Gd=Gd, G=G, E=E)


def b64(hs_pot, BT2, xs, dt):
    """Bs [n, 2, M, M] of one walker's fields xs [n, K]."""
    return numpy.array([itcf_ref.b_generic(hs_pot, BT2, x, dt) for x in xs])


def sums64(wins, wt):
    """(energies [3], denominator, one_rdm [2, M, M]) of per-walker windows; a walker with weight zero, or whose S is
    zero or not finite, does not count."""
    E = numpy.zeros(3, dtype=complex)
    den = 0j
    G = None
    for win, w in zip(wins, wt):
        if w == 0 or win is None or win['S'] == 0 or not numpy.isfinite(win['S']):
            continue
        den = den + w
        G = w * win['G'] if G is None else G + w * win['G']
        if win['E'] is not None:
            E = E + w * win['E']
    return E, den, G


# ---------------------------------------------------------------------------------------------------- extended
def det_ext(A):
    """Determinants of a stack [..., n, n]: Gaussian elimination with partial pivoting."""
    A = X.ext(A).copy()
    n = A.shape[-1]
    lead = A.shape[:-2]
    nb = int(numpy.prod(lead, dtype=int))
    W = A.reshape((nb, n, n))
    b = numpy.arange(nb)
    det = numpy.ones(nb, dtype=CLD)
    for c in range(n):
        p = c + numpy.argmax(numpy.abs(W[:, c:, c]), axis=1)
        swap = p != c
        top = W[b, c].copy()
        W[b, c] = W[b, p]
        W[b, p] = top
        det = numpy.where(swap, -det, det) * W[:, c, c]
        f = W[:, c + 1:, c] / W[:, c, c][:, None]
        W[:, c + 1:] = W[:, c + 1:] - f[:, :, None] * W[:, c][:, None, :]
    return det.reshape(lead)


def vhs_ext(hs_pot, x, dt, chunk=64):
    """V = i sqrt(dt) sum_k x_k L_k of fields x [..., K] in extended precision, hs_pot [M*M, K] taken a few vectors at
    a time (the whole of it in longdouble would be four times its size)."""
    x = X.ext(x)
    MM, K = hs_pot.shape
    M = int(round(MM ** 0.5))
    out = numpy.zeros(x.shape[:-1] + (MM,), dtype=CLD)
    for k0 in range(0, K, chunk):
        out = out + x[..., k0:k0 + chunk] @ X.ext(hs_pot[:, k0:k0 + chunk]).T
    return ((1j * numpy.sqrt(LD(dt))) * out).reshape(x.shape[:-1] + (M, M))


def b_ext(hs_pot, BT2, x, dt):
    BT2 = X.ext(BT2)
    E = X.exponentiate_matrix(vhs_ext(hs_pot, x, dt))
    return numpy.array([BT2[0] @ E @ BT2[0], BT2[1] @ E @ BT2[1]])


def energy_ext(H1, ecore, G, chol):
    """energy64 for a stack G [..., 2, M, M]."""
    H1, G, chol = X.ext(H1), X.ext(G), X.ext(chol)
    M = G.shape[-1]
    K = chol.shape[-1]
    lead = G.shape[:-3]
    e1b = numpy.sum(H1 * G, axis=(-3, -2, -1))
    Xs = G.reshape(lead + (2, M * M)) @ chol                       # [..., 2, K]
    ecoul = numpy.sum((Xs[..., 0, :] + Xs[..., 1, :]) ** 2, axis=-1)
    cv = chol.reshape(M, M, K)
    exx = 0
    for s in range(2):
        T = numpy.einsum('...il,ikn->...lkn', G[..., s, :, :], cv)
        exx = exx + numpy.einsum('...lkn,...kln->...', T, T)
    e2b = (ecoul - exx) / LD(2)
    return numpy.stack([e1b + e2b + LD(ecore), e1b + LD(ecore), e2b], axis=-1)


def window_ext(hs_pot, BT2, dt, xs, phi_old, dets, coeffs, na, nstblz, energy=None):
    """A stack of walkers: xs [n, nw, K], phi_old [nw, M, ne] -> dict(w [nw, nd], S [nw], G [nw, 2, M, M],
    E [nw, 3] or None)."""
    xs = numpy.asarray(xs)
    n, nw = xs.shape[:2]
    Bs = [b_ext(hs_pot, BT2, x, dt) for x in xs]                   # [2, nw, M, M] each
    right = X.spins(phi_old, na)
    nd = len(dets)
    ov, logr, Gd = [], [], []
    for d in range(nd):
        D = numpy.broadcast_to(X.ext(dets[d]), (nw,) + dets[d].shape)
        left = X.spins(D, na)
        lr = numpy.zeros(nw, dtype=LD)
        for i in range(n):
            t = n - 1 - i
            left = [X.dagger(Bs[t][s]) @ left[s] for s in range(2)]
            if i != 0 and i % nstblz == 0:
                for s in range(2):
                    if left[s].shape[-1]:
                        Q = X.reortho(left[s])
                        R = X.dagger(Q) @ left[s]
                        lr = lr + numpy.sum(numpy.log(numpy.diagonal(R, axis1=-2, axis2=-1).real), axis=-1)
                        left[s] = Q
        o = numpy.ones(nw, dtype=CLD)
        g = []
        for s in range(2):
            o = o * det_ext(X.dagger(left[s]) @ right[s])
            g.append(numpy.swapaxes(X.gab(left[s], right[s]), -1, -2))
        ov.append(o)
        logr.append(lr)
        Gd.append(numpy.stack(g, axis=1))                           # [nw, 2, M, M]
    logr = numpy.array(logr)
    with numpy.errstate(all='ignore'):
        w = (numpy.conj(X.ext(coeffs))[:, None] * numpy.exp(logr - numpy.max(logr, axis=0)) * numpy.array(ov)).T
    w = numpy.where(numpy.isfinite(w), w, 0)                        # [nw, nd]
    S = numpy.sum(w, axis=1)
    Gd = numpy.array(Gd)                                            # [nd, nw, 2, M, M]
    G = numpy.einsum('wd,dwsij->wsij', w, Gd) / S[:, None, None, None]
    E = None
    if energy is not None:
        Ed = numpy.array([energy_ext(energy[0], energy[1], Gd[d], energy[2]) for d in range(nd)])
        E = numpy.einsum('wd,dwk->wk', w, Ed) / S[:, None]
    return dict(w=w, S=S, G=G, E=E)


def sums_ext(hs_pot, BT2, dt, xs, phi_old, dets, coeffs, na, nstblz, wt, energy=None):
    """(energies, denominator, one_rdm, detw [nw, nd] normalised) in extended precision over the walkers given (all of
    them with a weight)."""
    win = window_ext(hs_pot, BT2, dt, xs, phi_old, dets, coeffs, na, nstblz, energy)
    wt = X.ext(wt)
    G = numpy.einsum('w,wsij->sij', wt, win['G'])
    E = numpy.einsum('w,wk->k', wt, win['E']) if energy is not None else numpy.zeros(3, dtype=CLD)
    return E, numpy.sum(wt), G, win['w'] / win['S'][:, None]


def sums_ext_pool(hs_pot, BT2, dt, xs, phi_old, dets, coeffs, na, nstblz, wt, energy=None, nproc=1):
    """sums_ext with the walkers dealt over nproc worker processes (fresh interpreters that import numpy alone)."""
    nw = len(wt)
    if nproc <= 1 or nw <= 1:
        return sums_ext(hs_pot, BT2, dt, xs, phi_old, dets, coeffs, na, nstblz, wt, energy)
    per = -(-nw // nproc)
    chunks = [slice(i, min(nw, i + per)) for i in range(0, nw, per)]
    args = [(hs_pot, BT2, dt, xs[:, c], phi_old[c], dets, coeffs, na, nstblz, wt[c], energy) for c in chunks]
    with ProcessPoolExecutor(len(chunks), mp_context=multiprocessing.get_context('spawn')) as pool:
        parts = list(pool.map(sums_ext, *zip(*args)))
    return (sum(p[0] for p in parts), sum(p[1] for p in parts), sum(p[2] for p in parts),
            numpy.concatenate([p[3] for p in parts]))


# ---------------------------------------------------------------------------------------------------- the rule
def slices(E, G, detw=None):
    """The slices a window is compared on: the one-body RDM sum per spin, the three energy sums, the weights."""
    out = [numpy.asarray(G[0]).ravel(), numpy.asarray(G[1]).ravel(), numpy.asarray(E).ravel()]
    if detw is not None:
        out.append(numpy.asarray(detw).ravel())
    return out


def slice_errors(got, want):
    """max |got - want| over a slice / max(1, max |want| over it), in extended precision (itcf_ref_ext.slice_errors'
    scale on this window's slices)."""
    errs = []
    for g, w in zip(got, want):
        g, w = X.ext(g), X.ext(w)
        assert g.shape == w.shape, (g.shape, w.shape)
        if g.size == 0:
            errs.append(0.0)
            continue
        errs.append(float(numpy.max(numpy.abs(g - w)) / numpy.maximum(LD(1), numpy.max(numpy.abs(w)))))
    return numpy.array(errs)


EXT_COST = 2.5e-7        # seconds of one core per walker, step and M^3 (tests/itcf_models.py)
SAMPLE = 4


def compare(case, got, hs_pot, BT2, dt, xs, phi_old, dets, coeffs, na, nstblz, wt, energy=None, sample=False, path=''):
    """The rule of tests/itcf_ref_ext.py on one window: got = (energies, denominator, one_rdm, detw) of
    AfqDevice.bp_update_msd, xs [n, nw, K] the fields read back from the device, wt [nw] the weight of every walker in
    the window (0: it does not count).  err_ref is the largest slice error of the fp64 restatement's sums against the
    extended restatement's; the device passes when every slice of its sums (and of its normalised weights) is within
    bound(err_ref) of the extended ones.  sample (M >= 100 with 64 or more walkers only): err_ref from SAMPLE live
    walkers (first, last and two between), and the device's sums over all walkers against the fp64 restatement's."""
    E, den, G, detw = got
    xs = numpy.asarray(xs)
    nw, M = phi_old.shape[0], phi_old.shape[-2]
    wt = numpy.asarray(wt, dtype=complex)
    live = [w for w in range(nw) if wt[w] != 0]
    assert not sample or (M >= 100 and nw >= 64), "only M >= 100 with 64 or more walkers may be sampled"
    use = live
    if sample and len(live) > SAMPLE:
        use = [live[(len(live) - 1) * k // (SAMPLE - 1)] for k in range(SAMPLE)]
    wins = {w: window64(b64(hs_pot, BT2, xs[:, w], dt), phi_old[w], dets, coeffs, na, nstblz, energy)
            for w in (live if sample else use)}
    E64, den64, G64 = sums64([wins[w] for w in use], wt[use])
    w64 = numpy.array([wins[w]['w'] / wins[w]['S'] for w in use])
    cost = EXT_COST * len(xs) * M ** 3 * len(use)
    nproc = min(12, len(use)) if cost > 4.0 else 1
    Ex, denx, Gx, wx = sums_ext_pool(hs_pot, BT2, dt, xs[:, use], phi_old[use], dets, coeffs, na, nstblz, wt[use],
                                     energy, nproc)
    err_ref = float(numpy.max(slice_errors(slices(E64, G64, w64), slices(Ex, Gx, wx))))
    limit = X.bound(err_ref)
    sampled = sample and len(live) > SAMPLE
    if sampled:
        Ew, denw, Gw = sums64([wins[w] for w in live], wt[live])
        want = slices(Ew, Gw, numpy.array([wins[w]['w'] / wins[w]['S'] for w in live]))
        have = slices(E, G, detw[live])
    else:
        want = slices(Ex, Gx, wx)
        have = slices(E, G, detw[use])
    err = slice_errors(have, want)
    worst = float(numpy.max(err))
    print("BPMSD-CASE | %s | M=%d nw=%d live=%d ndet=%d n=%d nstblz=%d | err_ref %.2e | device %.2e | bound %.2e | ratio %.3f | %s | %s"
          % (case, M, nw, len(live), len(dets), len(xs), nstblz, err_ref, worst, limit, worst / limit,
             'sampled %d, device vs fp64' % SAMPLE if sampled else 'extended', path))
    den_want = complex(numpy.sum(wt))
    assert abs(den - den_want) <= 1e-12 * max(1.0, abs(den_want)), (den, den_want)
    assert numpy.isfinite(G).all() and numpy.isfinite(E).all()
    # a model whose fp64 restatement is already this far off is badly conditioned: change the model, not the rule
    assert err_ref <= 1e-13, err_ref
    assert worst <= limit, (case, err.tolist(), limit)
    return err_ref, worst, limit
