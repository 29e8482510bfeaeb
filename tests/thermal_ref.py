"""fp64 numpy / scipy restatement of the finite-temperature Hubbard path with discrete Hirsch fields (DESIGN.md 4,
"thermal walkers"), written from the formulas, for a population of nw walkers at once:

  stack      nbins = L / stack_size bins per walker and spin; a fresh path has BT^stack_size in every bin (BT the
             trial's density matrix, left-multiplied stack_size times); slice number `time_slice` replaces
             (in-bin counter == 0) or left-multiplies bin time_slice // stack_size by B_s = diag(BV_s) BH1_s
  G          G_s = [I + A]^-1, A the product of the bins starting behind bin slice_ix // stack_size and wrapping round,
             by the stratified decomposition  Q D T = B_first (column-pivoted QR), C = (B Q) D, Q D t = C, T <- t T,
             G = T^-1 (D_b Q^T T^-1 + D_s)^-1 D_b Q^T,  D_b = 1 / |D|, D_s = sign(D) where |D| > 1, else D_b = 1, D_s = D
  slice      for the sites i in order: probs_x = 1/2 prod_s (1 + (1 - G_s[i,i]) (auxf[x,s] - 1)), p = max(probs, 0),
             norm = p_0 + p_1; norm > 0: weight *= norm exp(eshift), x = 0 if u_i < p_0 / norm else 1,
             G_s -= (auxf[x,s] - 1) G_s[:, i] (e_i - G_s[i, :]) / (1 + (1 - G_s[i,i]) (auxf[x,s] - 1)), BV[s, i] = auxf[x, s];
             else weight = 0, G untouched (BV[s, i] then is auxf[0, s] here; such a walker contributes to nothing)
  refresh    after the slice, when time_slice % nstblz == 0: G from the stack at slice_ix = time_slice - 1
  wrap       then, when time_slice < L: G_s <- BT_s G_s BT_s^-1
  energy     P_s = I - G_s^T; T = sum_s sum_ij H1_s[i,j] P_s[i,j], V = U sum_i P_up[i,i] P_down[i,i], nav = tr P_up + tr P_down

The path logic (Path) takes the number type and the two linear-algebra routines it needs (the stratified G of a chain
of bins, the product) from a `kit`; tests/thermal_ref_ext.py runs it in numpy.longdouble with its own routines."""
import numpy
import scipy.linalg


def split_d(D):
    """(D_b, D_s) of the graded diagonal D [..., M]."""
    big = numpy.abs(D) > 1
    safe = numpy.where(big, numpy.abs(D), 1)
    return numpy.where(big, 1 / safe, 1), numpy.where(big, numpy.sign(D), D)


def strat_greens_one(bins):
    """G of one chain of bins [B_first, ...] (each [M, M]), LAPACK's pivoted QR and inverses."""
    M = bins[0].shape[-1]
    Q, R, P = scipy.linalg.qr(bins[0], pivoting=True, check_finite=False)
    D = R.diagonal().copy()
    T = numpy.zeros((M, M))
    T[:, P] = R / D[:, None]
    for B in bins[1:]:
        C = (B @ Q) * D[None, :]
        Q, R, P = scipy.linalg.qr(C, pivoting=True, check_finite=False)
        D = R.diagonal().copy()
        t = numpy.zeros((M, M))
        t[:, P] = R / D[:, None]
        T = t @ T
    Db, Ds = split_d(D)
    Tinv = scipy.linalg.inv(T, check_finite=False)
    right = Db[:, None] * Q.T
    C = right @ Tinv + numpy.diag(Ds)
    return Tinv @ scipy.linalg.inv(C, check_finite=False) @ right


def strat_greens(bins):
    """bins: list of [nb, M, M] stacks in chain order -> G [nb, M, M]."""
    return numpy.array([strat_greens_one([B[b] for B in bins]) for b in range(bins[0].shape[0])])


class Kit64(object):
    dtype = numpy.float64
    strat_greens = staticmethod(strat_greens)

    @staticmethod
    def inv(A):
        return numpy.linalg.inv(A)


def chain_order(slice_ix, stack_size, nbins):
    """Bins of the chain for the Green's function at slice_ix, rightmost factor first."""
    bin_ix = slice_ix // stack_size
    if bin_ix == nbins:
        bin_ix = -1
    return [(bin_ix + i) % nbins for i in range(1, nbins + 1)]


def hubbard_auxf(U, dt, mu_system, mu_trial):
    """auxf [field, spin] of the spin decomposition with the chemical-potential shift (non-symmetric convention)."""
    gamma = numpy.arccosh(numpy.exp(0.5 * dt * U))
    auxf = numpy.array([[numpy.exp(gamma), numpy.exp(-gamma)], [numpy.exp(-gamma), numpy.exp(gamma)]])
    auxf = auxf * numpy.exp(-0.5 * dt * U)
    dmu = -(mu_system - mu_trial)
    return auxf * numpy.exp(-dt * dmu)


class Path(object):
    """nw walkers on one imaginary-time path of L slices."""

    def __init__(self, BT, BH1, auxf, L, stack_size, nstblz, nw, kit=Kit64, BT_inv=None):
        self.kit = kit
        dt = kit.dtype
        self.BT = numpy.asarray(BT, dtype=dt)
        self.BT_inv = kit.inv(self.BT) if BT_inv is None else numpy.asarray(BT_inv, dtype=dt)
        self.BH1 = numpy.asarray(BH1, dtype=dt)
        self.auxf = numpy.asarray(auxf, dtype=dt)
        assert L % stack_size == 0
        self.L, self.stack_size, self.nstblz, self.nw = L, stack_size, nstblz, nw
        self.nbins = L // stack_size
        self.M = self.BT.shape[-1]
        self.min_margin = numpy.inf
        self.unscaled = numpy.ones(nw, dtype=dt)        # (a reset leaves it alone)
        self.total_weight = dt(nw)
        self.reset()

    def reset(self):
        M, dt = self.M, self.kit.dtype
        pw = numpy.array([numpy.eye(M, dtype=dt)] * 2)
        for _ in range(self.stack_size):
            pw = self.BT @ pw
        self.stack = numpy.broadcast_to(pw, (self.nw, self.nbins, 2, M, M)).copy()
        self.time_slice = self.block = self.counter = 0
        self.weight = numpy.ones(self.nw, dtype=dt)
        G0 = self.greens_of(self.stack[:1], 0)
        self.G = numpy.broadcast_to(G0[0], (self.nw, 2, M, M)).copy()

    def greens_of(self, stack, slice_ix):
        """G [n, 2, M, M] of stack [n, nbins, 2, M, M] at slice_ix."""
        n, M = stack.shape[0], self.M
        bins = [stack[:, b].reshape(n * 2, M, M) for b in chain_order(slice_ix, self.stack_size, self.nbins)]
        return self.kit.strat_greens(bins).reshape(n, 2, M, M)

    def sites(self, u, eshift=0.0):
        """The M single-site updates of one slice -> (fields [nw, M], BV [nw, 2, M])."""
        dt = self.kit.dtype
        nw, M = self.nw, self.M
        u = numpy.asarray(u, dtype=dt)
        delta = self.auxf - 1
        fields = numpy.full((nw, M), -1, dtype=numpy.int32)
        BV = numpy.broadcast_to(self.auxf[0][None, :, None], (nw, 2, M)).copy()
        G = self.G
        ex = numpy.exp(dt(eshift))
        for i in range(M):
            g = G[:, :, i, i]                                                    # [nw, spin]
            probs = dt(0.5) * numpy.prod(1 + (1 - g)[:, None, :] * delta[None, :, :], axis=2)   # [nw, field]
            p = numpy.maximum(probs, 0)
            norm = p[:, 0] + p[:, 1]
            ok = norm > 0
            safe = numpy.where(ok, norm, 1)
            self.weight = numpy.where(ok, self.weight * norm * ex, 0)
            thr = p[:, 0] / safe
            x = numpy.where(u[:, i] < thr, 0, 1)
            if ok.any():
                self.min_margin = min(self.min_margin, float(numpy.min(numpy.abs(u[:, i] - thr)[ok])))
            d = delta[x]                                                         # [nw, spin]
            col = G[:, :, :, i]
            row = -G[:, :, i, :].copy()
            row[:, :, i] += 1
            f = d / (1 + (1 - g) * d)
            Gn = G - f[:, :, None, None] * col[:, :, :, None] * row[:, :, None, :]
            G = numpy.where(ok[:, None, None, None], Gn, G)
            BV[ok, :, i] = self.auxf[x[ok]]
            fields[ok, i] = x[ok]
        self.G = G
        return fields, BV

    def step(self, u, eshift=0.0):
        """One time slice with refresh and wrap -> fields [nw, M]."""
        fields, BV = self.sites(u, eshift)
        B = BV[:, :, :, None] * self.BH1[None]                                   # [nw, 2, M, M]
        if self.counter == 0:
            self.stack[:, self.block] = B
        else:
            self.stack[:, self.block] = B @ self.stack[:, self.block]
        self.time_slice += 1
        self.block = self.time_slice // self.stack_size
        self.counter = (self.counter + 1) % self.stack_size
        if self.time_slice % self.nstblz == 0:
            self.G = self.greens_of(self.stack, self.time_slice - 1)
        if self.time_slice < self.L:
            self.G = self.BT[None] @ self.G @ self.BT_inv[None]
        return fields

    def cap(self, frac=0.1):
        """|w| > frac total_weight -> frac total_weight, total_weight the last comb's (the population size before)."""
        cap = frac * self.total_weight
        self.weight = numpy.where(numpy.abs(self.weight) > cap, cap, self.weight)

    def pop_control(self, r):
        """The comb at the uniform r: rescale to the target nw, clone j-th walker of multiplicity > 1 over the j-th of
        multiplicity 0 (one copy per parent), every weight back to 1."""
        if self.nw == 1:
            return None
        a = numpy.abs(self.weight)
        total = numpy.sum(a)
        scale = total / self.nw
        self.total_weight = total
        self.unscaled = self.weight.copy()
        mult, pairs = comb_plan(a / scale, r, self.nw)
        for c, k in pairs:
            self.G[k] = self.G[c]
            self.stack[k] = self.stack[c]
            self.unscaled[k] = self.unscaled[c]
        self.weight = numpy.ones(self.nw, dtype=self.kit.dtype)
        return mult

    def estimator_row(self, H1, U):
        """[WeightFactor, Weight, ENumer, EDenom, ETotal, E1Body, E2Body, EHybrid, Overlap, Nav] of the population
        now: G rebuilt from the stack at the current time slice, sums in walker order."""
        G = self.greens_of(self.stack, self.time_slice)
        E, nav = energy(G, H1, U, self.kit.dtype)
        w = self.weight
        wsum = numpy.sum(w)
        enumer = numpy.sum(w * E[:, 0])
        return numpy.array([numpy.sum(self.unscaled), wsum, enumer, wsum, enumer / wsum, numpy.sum(w * E[:, 1]) / wsum,
                            numpy.sum(w * E[:, 2]) / wsum, 0.0, 1.0, numpy.sum(w * nav) / wsum], dtype=numpy.float64)

    def run(self, draws, npaths, npop_control, H1, U):
        """The driver's loop over npaths paths fed from the recorded stream `draws` (site uniforms in walker order,
        the comb's r where one is due) -> (rows [npaths + 1, 10], draws consumed)."""
        pos = 0
        n = self.nw * self.M
        rows = [self.estimator_row(H1, U)]
        for _ in range(npaths):
            for ts in range(self.L):
                self.step(numpy.asarray(draws[pos:pos + n]).reshape(self.nw, self.M))
                pos += n
                if ts > 0:
                    self.cap()
                if ts % npop_control == 0 and ts != 0 and self.nw > 1:
                    self.pop_control(draws[pos])
                    pos += 1
            rows.append(self.estimator_row(H1, U))
            self.reset()
        return numpy.array(rows), pos

    def energy(self, H1, U):
        """(E [nw, 3] = (E, T, V), nav [nw]) of the current G."""
        return energy(self.G, H1, U, self.kit.dtype)


def energy(G, H1, U, dtype=numpy.float64):
    M = G.shape[-1]
    P = numpy.eye(M, dtype=dtype) - numpy.swapaxes(G, -1, -2)
    ke = numpy.sum(numpy.asarray(H1.real, dtype=dtype)[None] * P, axis=(1, 2, 3))
    d = numpy.diagonal(P, axis1=-2, axis2=-1)
    pe = dtype(U) * numpy.sum(d[:, 0] * d[:, 1], axis=-1)
    nav = numpy.sum(d, axis=(1, 2))
    return numpy.stack([ke + pe, ke, pe], axis=1), nav


def comb_plan(weights, r, target):
    """parent multiplicities and the (clone, kill) pairs of the comb at the uniform r (weights already scaled)."""
    nw = len(weights)
    total = numpy.sum(weights)
    cprobs = numpy.cumsum(weights)
    mult = numpy.zeros(nw, dtype=numpy.int32)
    iw = 0
    for ic in range(int(target)):
        tooth = (ic + r) * (total / target)
        while not tooth < cprobs[iw]:
            iw += 1
        mult[iw] += 1
    kill = numpy.where(mult == 0)[0]
    clone = numpy.where(mult > 1)[0]
    return mult, list(zip(clone, kill))


# ---- a small Hubbard lattice and a one-body trial density matrix for the tests that need no fixture
def hubbard_kinetic(nx, ny, t=1.0):
    """Nearest-neighbour hopping of an nx x ny lattice with periodic boundaries (a bond is counted once)."""
    M = nx * ny
    T = numpy.zeros((M, M))
    for ix in range(nx):
        for iy in range(ny):
            i = ix * ny + iy
            for jx, jy in ((ix + 1) % nx, iy), (ix, (iy + 1) % ny):
                j = jx * ny + jy
                if i != j:
                    T[i, j] = T[j, i] = -t
    return T


def one_body_dmat(H1, mu, dt):
    """BT = expm(-dt (H1 - mu I)) per spin, and its inverse."""
    M = H1.shape[-1]
    BT = numpy.array([scipy.linalg.expm(-dt * (H1[s] - mu * numpy.eye(M))) for s in range(2)])
    BTinv = numpy.array([scipy.linalg.expm(dt * (H1[s] - mu * numpy.eye(M))) for s in range(2)])
    return BT, BTinv
