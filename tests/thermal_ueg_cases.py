"""Inputs shared by the thermal UEG tests: small electron gases with a one-body trial density matrix, the constants of
the plane-wave propagator restated from the formulas, random complex stacks, and the device set up on them."""
import numpy

from tests import thermal_ueg_ref as ur

ECUT_OF_M = {7: 0.5, 19: 1.0, 27: 1.5, 33: 2.0, 57: 2.5}


class Case(object):
    def __init__(self, ecut, ne, rs=1.0, beta=0.5, dt=0.05, mu=0.245, fb_bound=1.0):
        from pauxy_amd.systems import UEG
        from pauxy_amd.trial_density import OneBody
        self.system = UEG(rs, ne, ne, ecut, full_lists=True)
        self.system.mu = mu
        self.M, self.K, self.nq = self.system.nbasis, self.system.nfields, len(self.system.qvecs)
        self.dt, self.beta, self.mu, self.fb_bound = dt, beta, mu, fb_bound
        self.L = int(round(beta / dt))
        self.trial = OneBody(self.system, beta, dt)
        self.BT = numpy.array([self.trial.dmat[s].diagonal() for s in range(2)])
        self.BT_inv = numpy.array([self.trial.dmat_inv[s].diagonal() for s in range(2)])
        h = numpy.array([self.system.h1e_mod[s].diagonal() for s in range(2)])
        self.BH1 = numpy.exp(-0.5 * dt * h + 0.5 * dt * mu)
        self.ops = ur.Operators(self.system)
        self.mf_shift = ur.mf_shift_of(self.ops, self.BT)
        self._ops_ext = None

    @property
    def ops_ext(self):
        if self._ops_ext is None:
            from tests import thermal_ueg_ref_ext as ue
            self._ops_ext = ur.Operators(self.system, ue.KitExt)
        return self._ops_ext

    def full(self, d):
        """[2, M, M] of the diagonals [2, M]."""
        return numpy.array([numpy.diag(d[0]), numpy.diag(d[1])])

    def path64(self, stack_size, nw, **kw):
        return ur.Path(self.ops, kw.pop('BT', self.BT), kw.pop('BT_inv', self.BT_inv), kw.pop('BH1', self.BH1), self.dt,
                       self.L, stack_size, nw, mf_shift=kw.pop('mf_shift', self.mf_shift), fb_bound=self.fb_bound)

    def path_ext(self, stack_size, nw, **kw):
        from tests import thermal_ueg_ref_ext as ue
        return ue.path(self.ops_ext, kw.pop('BT', self.BT), kw.pop('BT_inv', self.BT_inv), kw.pop('BH1', self.BH1),
                       self.dt, self.L, stack_size, nw, mf_shift=kw.pop('mf_shift', self.mf_shift),
                       fb_bound=self.fb_bound)

    def random_stack(self, nw, nbins, stack_size, seed, spread=20.0):
        """[nw, nbins, 2, M, M] complex: every bin the product of stack_size factors diag(d) E diag(d), E the degree-6
        exponential of a random V = i (Hermitian) + (anti-Hermitian part) of the size of a plane-wave HS potential, d a
        one-body factor whose exponents spread over `spread` (the Hubbard test's recipe, made complex): at stack_size
        20 a bin has a condition number of 1e8."""
        rng = numpy.random.RandomState(seed)
        M = self.M
        e = numpy.linspace(-0.2 * spread, 0.8 * spread, M)
        d = numpy.exp(-0.5 * self.dt * e)
        eye = numpy.eye(M, dtype=numpy.complex128)
        stack = numpy.empty((nw, nbins, 2, M, M), dtype=numpy.complex128)
        for w in range(nw):
            for b in range(nbins):
                P = numpy.array([eye, eye])
                for _ in range(stack_size):
                    A = rng.normal(size=(M, M)) + 1j * rng.normal(size=(M, M))
                    V = 0.1 * numpy.sqrt(self.dt) * (1j * (A + A.conj().T) + 0.3 * (A - A.conj().T))
                    E, term = eye.copy(), eye.copy()
                    for n in range(1, 7):
                        term = V @ term / n
                        E = E + term
                    B = d[:, None] * E * d[None, :]
                    P = numpy.array([B @ P[0], (B * numpy.exp(0.01 * self.dt)) @ P[1]])
                stack[w, b] = P
        return stack

    def device(self, nw, stack_size, options=0, L=None, BT=None):
        from pauxy_amd.device import AfqDevice
        s = self.system
        dev = AfqDevice(0)
        try:
            dev.set_system_ueg(s.iA, s.iB, s.ikpq_i, s.ikpq_kpq, s.ipmq_i, s.ipmq_pmq, s.vqvec, s.vol,
                               numpy.array([s.H1[0].diagonal(), s.H1[1].diagonal()]), s.ecore, s.nup, s.ndown)
            dev.walkers_alloc(nw)
            dev.thermal_configure_continuous(self.L if L is None else L, stack_size, self.dt,
                                             self.full(self.BT) if BT is None else BT, self.full(self.BT_inv),
                                             self.full(self.BH1), self.mf_shift, self.fb_bound, options)
        except Exception:
            dev.close()
            raise
        return dev
