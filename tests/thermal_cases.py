"""Inputs shared by the thermal tests: small Hubbard lattices with a one-body trial density matrix, stacks built from
random field configurations, and the device set up on them."""
import numpy

from tests import thermal_ref as tr


class Case(object):
    def __init__(self, nx, ny, U, dt, mu=1.0, mu_trial=None):
        self.nx, self.ny, self.U, self.dt, self.mu = nx, ny, float(U), float(dt), float(mu)
        self.M = nx * ny
        T = tr.hubbard_kinetic(nx, ny)
        self.H1 = numpy.array([T, T])
        self.mu_trial = self.mu if mu_trial is None else float(mu_trial)
        self.BT, self.BT_inv = tr.one_body_dmat(self.H1, self.mu_trial, dt)
        self.BH1, _ = tr.one_body_dmat(self.H1, self.mu_trial, dt)
        self.auxf = tr.hubbard_auxf(self.U, dt, self.mu, self.mu_trial)
        self.na = self.nb = max(1, self.M // 2)

    def random_stack(self, nw, nbins, stack_size, seed):
        """[nw, nbins, 2, M, M]: every bin the product of stack_size propagators of random fields."""
        rng = numpy.random.RandomState(seed)
        M = self.M
        stack = numpy.empty((nw, nbins, 2, M, M))
        for w in range(nw):
            for b in range(nbins):
                P = numpy.array([numpy.eye(M), numpy.eye(M)])
                for _ in range(stack_size):
                    x = rng.randint(0, 2, M)
                    B = self.auxf[x].T[:, :, None] * self.BH1
                    P = B @ P
                stack[w, b] = P
        return stack

    def device(self, nw, L, stack_size, nstblz, options=0):
        from pauxy_amd.device import AfqDevice
        dev = AfqDevice(0)
        dev.set_system_hubbard(self.H1.astype(complex), self.U, self.na, self.nb)
        dev.walkers_alloc(nw)
        dev.thermal_configure(L, stack_size, nstblz, self.BT, self.BT_inv, self.BH1, self.auxf, options)
        return dev

    def h1_scale(self):
        """||H1||_1 + U M: what an energy or nav, linear in G, may amplify an error of G by."""
        return float(numpy.max(numpy.sum(numpy.abs(self.H1[0]), axis=0))) + self.U * self.M
