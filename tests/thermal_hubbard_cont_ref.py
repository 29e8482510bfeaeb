"""Restatement of the finite-temperature path of the Hubbard model with continuous fields ("thermal
walkers, continuous fields, dense trial"), written from the formulas, for a population of nw walkers at once, in fp64
(thermal_ueg_ref.Kit64) or in numpy.clongdouble (thermal_ueg_ref_ext.KitExt):

  setup      P_T = I - G_T^T of the trial's ONE-slice G_T = [I + BT]^-1; mf_shift_i = i sqrt(U) (P_T,up,ii + P_T,dn,ii);
             mf_core = mf_shift . mf_shift / 2; mf_const_fac = exp(-dt mf_core);
             BH1_s = expm(-dt/2 (h1e_mod_s - i sqrt(U) diag(mf_shift) - mu)) -- dense and real
  fields     P = I - G^T; vbias_i = i sqrt(U) (P_up,ii + P_dn,ii); xbar = -sqrt(dt) (vbias - mf_shift), components with
             |xbar| > 1 scaled to unit modulus and counted; xs = xi - xbar; cmf = -sqrt(dt) xs . mf_shift;
             cfb = xi . xbar - xbar . xbar / 2 (unconjugated dots)
  slice      v = sqrt(dt) i sqrt(U) xs; bv = sum_{n <= 6} v^n / n! by t <- v t / n; B_s = BH1_s (diag(bv) BH1_s)
  stack      at in-bin counter 0 right <- I and left <- BT^stack_size (BT left-multiplied stack_size times onto I);
             left <- left BT_inv; right_s <- B_s right_s; bin[block]_s = left_s right_s
  G, reset   as tests/thermal_ueg_ref.py, every fresh bin the dense BT^stack_size
  weight     as tests/thermal_ueg_ref.py with magn = |mf_const_fac exp(hyb)|
  energy     estimators/hubbard.py:93-114 on P (tests/thermal_ref.energy), nav = tr P_up + tr P_dn

The path logic is thermal_ueg_ref.Path's; this module overrides what the dense trial and the diagonal field
exponential change."""
import numpy
import scipy.linalg

from tests import thermal_ref, thermal_ueg_ref
from tests.thermal_ueg_ref import Kit64


def constants(T, U, mu, dt, BT):
    """(BH1 [2, M, M] real, mf_shift [M] complex, mf_core, mf_const_fac) in fp64, from the kinetic matrix T [M, M], the
    system's mu and the trial's BT [2, M, M]."""
    M = T.shape[-1]
    eye = numpy.eye(M)
    P = numpy.array([eye - scipy.linalg.inv(eye + BT[s]).T for s in range(2)])
    iu = 1j * U ** 0.5
    mf_shift = iu * (numpy.diag(P[0]) + numpy.diag(P[1]))
    mf_core = 0.5 * numpy.dot(mf_shift, mf_shift)
    h1e_mod = T - 0.5 * U * eye
    H1 = h1e_mod - (iu * numpy.diag(mf_shift) + mu * eye)
    BH1 = scipy.linalg.expm(-0.5 * dt * H1)
    assert numpy.max(numpy.abs(BH1.imag)) == 0.0
    return numpy.array([BH1.real, BH1.real]), mf_shift, mf_core, numpy.exp(-dt * mf_core)


class Path(thermal_ueg_ref.Path):
    """nw walkers on one imaginary-time path of L slices; BT, BT_inv, BH1 dense real [2, M, M] (the fp64 numbers the
    device is given, so that both build left_k from the same numbers), H1 [2, M, M] and U for the energy."""

    def __init__(self, H1, U, BT, BT_inv, BH1, mf_shift, mf_const_fac, dt, L, stack_size, nw, kit=Kit64):
        self.kit = kit
        rt, ct = kit.rtype, kit.dtype
        self.H1, self.U = numpy.asarray(H1), U
        self.BT = numpy.asarray(BT, dtype=rt)
        self.BT_inv = numpy.asarray(BT_inv, dtype=rt)
        self.BH1 = numpy.asarray(BH1, dtype=rt)
        assert L % stack_size == 0
        self.dt, self.sqrt_dt = rt(dt), rt(dt) ** rt(0.5)
        self.sqrt_u = rt(U) ** rt(0.5)
        self.L, self.stack_size, self.nw = L, stack_size, nw
        self.nbins = L // stack_size
        self.M = self.BT.shape[-1]
        pw = numpy.broadcast_to(numpy.eye(self.M, dtype=rt), self.BT.shape).copy()
        for _ in range(stack_size):
            pw = self.BT @ pw
        self.BTpow = pw
        self.left_table = []                                        # left_k, k = 0 .. stack_size - 1
        lf = pw
        for _ in range(stack_size):
            lf = lf @ self.BT_inv
            self.left_table.append(lf)
        self.mf_shift = numpy.asarray(mf_shift, dtype=ct)
        self.mf_const_fac = ct(mf_const_fac)
        self.min_cos_margin = numpy.inf
        self.nclip = 0
        self.ncap = 0
        self.nkill = 0
        self.unscaled = numpy.ones(nw, dtype=rt)
        self.total_weight = rt(nw)
        self.M0 = None
        self.reset(m0=True)
        self.G0, self.M00 = self.G[0].copy(), self.M0[0].copy()

    def reset(self, m0=False):
        M, ct = self.M, self.kit.dtype
        eye = numpy.eye(M, dtype=ct)
        bins = numpy.asarray(self.BTpow, dtype=ct)
        self.stack = numpy.broadcast_to(bins, (self.nw, self.nbins, 2, M, M)).copy()
        self.right = numpy.broadcast_to(eye, (self.nw, 2, M, M)).copy()
        self.time_slice = self.block = self.counter = 0
        self.weight = numpy.ones(self.nw, dtype=self.kit.rtype)
        G0 = self.greens_of(self.stack[:1], 0)
        self.G = numpy.broadcast_to(G0[0], (self.nw, 2, M, M)).copy()
        if m0 or self.M0 is None:
            self.M0 = numpy.broadcast_to(self.kit.det(G0[0]), (self.nw, 2)).copy()

    def fields(self, xi):
        ct = self.kit.dtype
        xi = numpy.asarray(xi, dtype=self.kit.rtype)
        d = 1 - numpy.diagonal(self.G, axis1=-2, axis2=-1)          # diagonal of P = I - G^T  [nw, 2, M]
        vbias = ct(1j) * self.sqrt_u * (d[:, 0] + d[:, 1])
        xbar = -self.sqrt_dt * (vbias - self.mf_shift[None])
        a = numpy.abs(xbar)
        clip = a > 1
        self.nclip += int(numpy.sum(clip))
        xbar = numpy.where(clip, xbar / numpy.where(clip, a, 1), xbar)
        xs = xi - xbar
        cmf = -self.sqrt_dt * (xs @ self.mf_shift)
        cfb = numpy.sum(xi * xbar, axis=1) - numpy.sum(xbar * xbar, axis=1) / 2
        return xbar, xs, cmf, cfb

    def bv_of(self, xs):
        v = self.sqrt_dt * (self.kit.dtype(1j) * self.sqrt_u) * xs
        t = numpy.ones_like(v)
        bv = numpy.ones_like(v)
        for n in range(1, 7):
            t = v * t / n
            bv = bv + t
        return bv

    def propagator(self, xs):
        """B [nw, 2, M, M] of the shifted fields."""
        bv = self.bv_of(xs)
        inner = bv[:, None, :, None] * self.BH1[None]               # BV BH1
        return self.BH1[None] @ inner

    def step(self, xi):
        xbar, xs, cmf, cfb = self.fields(xi)
        B = self.propagator(xs)
        if self.counter == 0:
            self.right = numpy.broadcast_to(numpy.eye(self.M, dtype=self.kit.dtype), B.shape).copy()
        left = self.left_table[self.counter]
        self.right = B @ self.right
        self.B = B
        self.stack[:, self.block] = left[None] @ self.right
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
        with numpy.errstate(over='ignore', invalid='ignore'):
            magn = numpy.abs(self.mf_const_fac * numpy.exp(hyb))
        if not magn < numpy.inf:                      # infinite, or not a number: the walker dies and keeps its M0
            self.weight[w] = 0
            return
        c = numpy.cos((hyb - cfb).imag)
        if not c < -1e-3:
            self.min_cos_margin = min(self.min_cos_margin, float(abs(c)))
        if not c > 0:
            self.nkill += 1
        self.weight[w] = self.weight[w] * magn * max(self.kit.rtype(0), c)
        self.M0[w] = Mnew

    def energy(self):
        return thermal_ref.energy(self.G, self.H1, self.U, self.kit.dtype)

    def estimator_row(self):
        G = self.greens_of(self.stack, self.time_slice)
        E, nav = thermal_ref.energy(G, self.H1, self.U, self.kit.dtype)
        E, nav = E.real, nav.real
        w = self.weight
        wsum = numpy.sum(w)
        enumer = numpy.sum(w * E[:, 0])
        return numpy.array([numpy.sum(self.unscaled), wsum, enumer, wsum, enumer / wsum, numpy.sum(w * E[:, 1]) / wsum,
                            numpy.sum(w * E[:, 2]) / wsum, 0.0, 1.0, numpy.sum(w * nav) / wsum], dtype=self.kit.rtype)


def path_ext(*args, **kw):
    """Path in extended precision."""
    from tests.thermal_ueg_ref_ext import KitExt
    return Path(*args, kit=KitExt, **kw)
