"""fp64 numpy / scipy restatement of the finite-temperature path of the uniform electron gas with continuous fields
("thermal walkers, continuous fields"), written from the formulas, for a population of nw walkers at once:

  fields     P = I - G^T; vbias = vec(P_up + P_dn) . [iA | iB]; xbar = -sqrt(dt) vbias, components with |xbar| > fb_bound
             scaled to unit modulus; xs = xi - xbar; cmf = -sqrt(dt) xs . mf_shift; cfb = xi . xbar - xbar . xbar / 2
             (unconjugated dots)
  slice      VHS = sqrt(dt) reshape(iA xs[:nq] + iB xs[nq:]); BV = sum_{n <= 6} VHS^n / n!;
             B_s = diag(d_s) BV diag(d_s), d_s the diagonal of BH1_s
  stack      at in-bin counter 0 right <- I; right_s <- B_s right_s; bin[block]_s = diag(left) right_s, where left starts
             a bin as BT^stack_size (BT applied stack_size times to 1) and is multiplied by BT_inv at every slice
  G          G_s = [I + bin[nbins - 1] .. bin[0]]^-1 by the stratified decomposition of tests/thermal_ref.py in complex
             arithmetic: D_b = 1 / |D|, D_s = D / |D| where |D| > 1, else D_b = 1, D_s = D
  weight     Mnew_s = det G_s; oratio = M0_up M0_dn / (Mnew_up Mnew_dn); hyb = log(oratio) + cfb + cmf;
             magn = |exp(hyb)|; a zero denominator or a magn that is not finite: weight = 0 and M0 kept; else
             weight *= magn max(0, cos Im(hyb - cfb)) and M0 = Mnew
  reset      bins = BT^stack_size, G the trial's, weight = 1.  M0 is NOT reset: the reference's Walkers.reset leaves
             walker.M0 at the determinant of the end of the previous path (walkers/handler.py:424-430), and the first
             slice of the next path divides by it; afq_thermal_reset does the same.  `reset(m0=True)` is a fresh
             population (afq_thermal_configure_continuous): M0 = det of the trial's G.
  energy     local_energy_ueg of P (estimators/ueg.py:27-88, lists over all plane waves), nav = tr P_up + tr P_dn

The path logic (Path) takes the number types and the two linear-algebra routines it needs (the stratified G of a chain
of bins, the determinant) from a `kit`; tests/thermal_ueg_ref_ext.py runs it in numpy.longdouble."""
import numpy
import scipy.linalg

from tests.thermal_ref import chain_order, comb_plan  # noqa: F401  (the same bins, the same comb)


def split_d(D):
    """(D_b, D_s) of the complex graded diagonal D [..., M]."""
    a = numpy.abs(D)
    big = a > 1
    safe = numpy.where(big, a, 1)
    return numpy.where(big, 1 / safe, 1), numpy.where(big, D / safe, D)


def strat_greens_one(bins):
    """G of one chain of complex bins [B_first, ...] (each [M, M]), LAPACK's pivoted QR and inverses."""
    M = bins[0].shape[-1]
    Q, R, P = scipy.linalg.qr(bins[0], pivoting=True, check_finite=False)
    D = R.diagonal().copy()
    T = numpy.zeros((M, M), dtype=numpy.complex128)
    T[:, P] = R / D[:, None]
    for B in bins[1:]:
        C = (B @ Q) * D[None, :]
        Q, R, P = scipy.linalg.qr(C, pivoting=True, check_finite=False)
        D = R.diagonal().copy()
        t = numpy.zeros((M, M), dtype=numpy.complex128)
        t[:, P] = R / D[:, None]
        T = t @ T
    Db, Ds = split_d(D)
    Tinv = scipy.linalg.inv(T, check_finite=False)
    right = Db[:, None] * Q.conj().T
    C = right @ Tinv + numpy.diag(Ds)
    return Tinv @ scipy.linalg.inv(C, check_finite=False) @ right


def strat_greens(bins):
    """bins: list of [nb, M, M] stacks in chain order -> G [nb, M, M]."""
    return numpy.array([strat_greens_one([numpy.asarray(B[b], dtype=numpy.complex128) for B in bins])
                        for b in range(bins[0].shape[0])])


class Kit64(object):
    dtype = numpy.complex128
    rtype = numpy.float64
    strat_greens = staticmethod(strat_greens)

    @staticmethod
    def det(A):
        return numpy.array([scipy.linalg.det(a, check_finite=False) for a in A.reshape((-1,) + A.shape[-2:])]
                           ).reshape(A.shape[:-2])


class Operators(object):
    """What the path needs of a plane-wave system, as dense arrays of the kit's type: iA, iB [M M, nq], the energy's
    index lists, vqvec, vol, the diagonal of H1."""

    def __init__(self, system, kit=Kit64):
        self.M, self.nq = system.nbasis, len(system.qvecs)
        self.iA = numpy.asarray(system.iA.toarray(), dtype=kit.dtype)
        self.iB = numpy.asarray(system.iB.toarray(), dtype=kit.dtype)
        self.lists = (system.ikpq_i, system.ikpq_kpq, system.ipmq_i, system.ipmq_pmq)
        self.vqvec = numpy.asarray(system.vqvec, dtype=kit.rtype)
        self.vol = kit.rtype(system.vol)
        self.H1diag = numpy.asarray(numpy.diagonal(system.H1, axis1=-2, axis2=-1).real, dtype=kit.rtype)


def mf_shift_of(ops, BTdiag, kit=None):
    """construct_mf_shift (planewave.py:83-89): from P = I - G^T of the trial's ONE-slice G = [I + BT]^-1
    (onebody.py:111), BT diagonal [2, M]."""
    kit = kit or Kit64
    M = ops.M
    bt = numpy.asarray(BTdiag, dtype=kit.rtype)
    p = 1 - 1 / (1 + bt)
    Pv = numpy.asarray(numpy.diag(p[0] + p[1]), dtype=kit.dtype).reshape(M * M)
    return numpy.concatenate([Pv @ ops.iA, Pv @ ops.iB])


def energy(ops, G):
    """(E [n, 3] = (E, T, V) complex, nav [n] complex) of G [n, 2, M, M]."""
    M = ops.M
    P = numpy.eye(M, dtype=G.dtype) - numpy.swapaxes(G, -1, -2)
    d = numpy.diagonal(P, axis1=-2, axis2=-1)                       # [n, 2, M]
    ke = numpy.sum(ops.H1diag[None] * d, axis=(1, 2))
    ki, kk, pi, pp = ops.lists
    n = G.shape[0]
    Gkpq = numpy.zeros((n, 2, ops.nq), dtype=G.dtype)
    Gpmq = numpy.zeros((n, 2, ops.nq), dtype=G.dtype)
    Gprod = numpy.zeros((n, 2, ops.nq), dtype=G.dtype)
    for q in range(ops.nq):
        if len(ki[q]):
            Gkpq[:, :, q] = numpy.sum(P[:, :, ki[q], kk[q]], axis=-1)
        if len(pi[q]):
            Gpmq[:, :, q] = numpy.sum(P[:, :, pi[q], pp[q]], axis=-1)
        if len(ki[q]) and len(pi[q]):
            a = P[:, :, pi[q][:, None], kk[q][None, :]]             # [n, 2, b, a]
            b = P[:, :, ki[q][None, :], pp[q][:, None]]
            Gprod[:, :, q] = numpy.sum(a * b, axis=(-1, -2))
    same = Gkpq * Gpmq - Gprod
    cross = Gkpq[:, 0] * Gpmq[:, 1] + Gkpq[:, 1] * Gpmq[:, 0]
    pe = (same[:, 0] + same[:, 1] + cross) @ ops.vqvec / (2 * ops.vol)
    return numpy.stack([ke + pe, ke, pe], axis=1), numpy.sum(d, axis=(1, 2))


class Path(object):
    """nw walkers on one imaginary-time path of L slices."""

    def __init__(self, ops, BTdiag, BTinvdiag, BH1diag, dt, L, stack_size, nw, kit=Kit64, mf_shift=None, fb_bound=1.0):
        self.kit, self.ops, self.fb_bound = kit, ops, fb_bound
        rt = kit.rtype
        self.BT = numpy.asarray(BTdiag, dtype=rt)                   # [2, M]
        self.BT_inv = numpy.asarray(BTinvdiag, dtype=rt)
        self.d = numpy.asarray(BH1diag, dtype=rt)
        assert L % stack_size == 0
        self.dt, self.sqrt_dt = rt(dt), rt(dt) ** rt(0.5)
        self.L, self.stack_size, self.nw = L, stack_size, nw
        self.nbins = L // stack_size
        self.M = ops.M
        pw = numpy.ones_like(self.BT)
        for _ in range(stack_size):
            pw = self.BT * pw
        self.BTpow = pw
        self.min_cos_margin = numpy.inf
        self.nclip = 0
        self.ncap = 0
        self.unscaled = numpy.ones(nw, dtype=rt)
        self.total_weight = rt(nw)
        self.M0 = None
        self.reset(m0=True)
        self.G0, self.M00 = self.G[0].copy(), self.M0[0].copy()
        self.mf_shift = mf_shift_of(ops, self.BT, kit) if mf_shift is None else numpy.asarray(mf_shift, dtype=kit.dtype)

    def reset(self, m0=False):
        M, ct = self.M, self.kit.dtype
        eye = numpy.eye(M, dtype=ct)
        bins = numpy.array([eye * self.BTpow[0][:, None], eye * self.BTpow[1][:, None]])
        self.stack = numpy.broadcast_to(bins, (self.nw, self.nbins, 2, M, M)).copy()
        self.right = numpy.broadcast_to(eye, (self.nw, 2, M, M)).copy()
        self.left = self.BTpow.copy()
        self.time_slice = self.block = self.counter = 0
        self.weight = numpy.ones(self.nw, dtype=self.kit.rtype)
        G0 = self.greens_of(self.stack[:1], 0)
        self.G = numpy.broadcast_to(G0[0], (self.nw, 2, M, M)).copy()
        if m0 or self.M0 is None:
            self.M0 = numpy.broadcast_to(self.kit.det(G0[0]), (self.nw, 2)).copy()

    def greens_of(self, stack, slice_ix):
        """G [n, 2, M, M] of stack [n, nbins, 2, M, M] at slice_ix."""
        n, M = stack.shape[0], self.M
        bins = [stack[:, b].reshape(n * 2, M, M) for b in chain_order(slice_ix, self.stack_size, self.nbins)]
        return self.kit.strat_greens(bins).reshape(n, 2, M, M)

    def fields(self, xi):
        """-> (xbar, xs [nw, K], cmf, cfb [nw]) of the current G."""
        ct, M = self.kit.dtype, self.M
        xi = numpy.asarray(xi, dtype=self.kit.rtype)
        P = numpy.eye(M, dtype=ct) - numpy.swapaxes(self.G, -1, -2)
        Pv = (P[:, 0] + P[:, 1]).reshape(self.nw, M * M)
        vbias = numpy.concatenate([Pv @ self.ops.iA, Pv @ self.ops.iB], axis=1)
        xbar = -self.sqrt_dt * vbias
        a = numpy.abs(xbar)
        clip = a > self.fb_bound
        self.nclip += int(numpy.sum(clip))
        xbar = numpy.where(clip, xbar / numpy.where(clip, a, 1), xbar)
        xs = xi - xbar
        cmf = -self.sqrt_dt * (xs @ self.mf_shift)
        cfb = numpy.sum(xi * xbar, axis=1) - numpy.sum(xbar * xbar, axis=1) / 2
        return xbar, xs, cmf, cfb

    def propagator(self, xs):
        """B [nw, 2, M, M] of the shifted fields."""
        ct, M, nq = self.kit.dtype, self.M, self.ops.nq
        VHS = self.sqrt_dt * (xs[:, :nq] @ self.ops.iA.T + xs[:, nq:] @ self.ops.iB.T).reshape(self.nw, M, M)
        eye = numpy.eye(M, dtype=ct)
        BV = numpy.broadcast_to(eye, VHS.shape).copy()
        term = BV.copy()
        for n in range(1, 7):
            term = VHS @ term / n
            BV = BV + term
        return self.d[None, :, :, None] * (BV[:, None] * self.d[None, :, None, :])

    def step(self, xi):
        """One time slice -> (xbar, cmf, cfb)."""
        xbar, xs, cmf, cfb = self.fields(xi)
        B = self.propagator(xs)
        if self.counter == 0:
            self.right = numpy.broadcast_to(numpy.eye(self.M, dtype=self.kit.dtype), B.shape).copy()
            self.left = self.BTpow.copy()
        self.left = self.left * self.BT_inv
        self.right = B @ self.right
        self.B = B
        self.stack[:, self.block] = self.left[None, :, :, None] * self.right
        self.time_slice += 1
        self.block = self.time_slice // self.stack_size
        self.counter = (self.counter + 1) % self.stack_size
        self.G = self.greens_of(self.stack, self.L)
        Mnew = self.kit.det(self.G)
        for w in range(self.nw):
            self.update_weight(w, Mnew[w], cmf[w], cfb[w])
        return xbar, cmf, cfb

    def update_weight(self, w, Mnew, cmf, cfb):
        den = Mnew[0] * Mnew[1]
        if den == 0:
            self.weight[w] = 0
            return
        oratio = self.M0[w, 0] * self.M0[w, 1] / den
        hyb = numpy.log(oratio) + cfb + cmf
        with numpy.errstate(over='ignore'):
            magn = numpy.exp(hyb.real)
        if not magn < numpy.inf:                      # infinite, or not a number: the walker dies and keeps its M0
            self.weight[w] = 0
            return
        c = numpy.cos((hyb - cfb).imag)
        if not c < -1e-3:
            self.min_cos_margin = min(self.min_cos_margin, float(abs(c)))
        self.weight[w] = self.weight[w] * magn * max(self.kit.rtype(0), c)
        self.M0[w] = Mnew

    def cap(self, frac=0.1):
        cap = frac * self.total_weight
        self.ncap += int(numpy.sum(numpy.abs(self.weight) > cap))
        self.weight = numpy.where(numpy.abs(self.weight) > cap, cap, self.weight)

    def pop_control(self, r):
        """The comb at the uniform r -> parent multiplicities; G, the bins, right and M0 travel with a clone."""
        if self.nw == 1:
            return None
        a = numpy.abs(self.weight)
        total = numpy.sum(a)
        self.total_weight = total
        self.unscaled = self.weight.copy()
        mult, pairs = comb_plan(a / (total / self.nw), r, self.nw)
        for c, k in pairs:
            self.G[k], self.stack[k], self.right[k], self.M0[k] = self.G[c], self.stack[c], self.right[c], self.M0[c]
            self.unscaled[k] = self.unscaled[c]
        self.weight = numpy.ones(self.nw, dtype=self.kit.rtype)
        return mult

    def energy(self):
        return energy(self.ops, self.G)

    def estimator_row(self):
        """[WeightFactor, Weight, ENumer, EDenom, ETotal, E1Body, E2Body, EHybrid, Overlap, Nav] (real parts)."""
        G = self.greens_of(self.stack, self.time_slice)
        E, nav = energy(self.ops, G)
        E, nav = E.real, nav.real
        w = self.weight
        wsum = numpy.sum(w)
        enumer = numpy.sum(w * E[:, 0])
        return numpy.array([numpy.sum(self.unscaled), wsum, enumer, wsum, enumer / wsum, numpy.sum(w * E[:, 1]) / wsum,
                            numpy.sum(w * E[:, 2]) / wsum, 0.0, 1.0, numpy.sum(w * nav) / wsum], dtype=self.kit.rtype)

    def run(self, xis, rs, npaths, npop_control):
        """The driver's loop: xis [npaths L, nw, K] the fields, rs the comb's uniforms in order ->
        (rows [npaths + 1, 10], weights [npaths L, nw] after every slice, before its cap, parents of every comb)."""
        rows, wts, parents = [self.estimator_row()], [], []
        it, ir = 0, 0
        for _ in range(npaths):
            for ts in range(self.L):
                self.step(xis[it])
                it += 1
                wts.append(self.weight.copy())
                if ts > 0:
                    self.cap()
                if ts % npop_control == 0 and ts != 0 and self.nw > 1:
                    parents.append(self.pop_control(rs[ir]))
                    ir += 1
            rows.append(self.estimator_row())
            self.reset()
        return numpy.array(rows), numpy.array(wts), parents
