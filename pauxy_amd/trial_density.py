"""One-body trial density matrix of the finite-temperature algorithm.

Mirrors pauxy/trial_density_matrices/onebody.py:15-113 and chem_pot.py:7-67 (``OneBody``: ``name = 'thermal'``,
``dmat``, ``dmat_inv``, ``mu``, ``nav``, ``stack_size``, ``num_slices``, ``num_bins``, ``cond``).  Host set-up only:
numpy / scipy, nothing on the device.

    dmat_s = expm(-dt H1_s) exp(dt mu)            (BT of the propagator and of the walkers' stack)
    mu     bisected until |<N>(mu) - nav| < threshold, <N>(mu) = sum_s tr [I + expm(beta (H1_s - mu))]^-1

<N>(mu) is evaluated in the eigenbasis of the Hermitian H1_s, where it is a sum of Fermi factors: stable at any beta,
no stratified product needed.  The bisection itself (bracket [-1, 1] widened by 2 on each side, midpoints, the
1e-6 threshold, at most 1000 iterations) is the reference's, so the chemical potential found is the same midpoint.
"""
import numpy
import scipy.linalg


def update_stack(stack_size, num_slices):
    """The divisor of num_slices nearest to stack_size (the lower one on a tie): utils/misc.py:142-159."""
    lower = upper = min(stack_size, num_slices)
    while num_slices % lower:
        lower -= 1
    while num_slices % upper:
        upper += 1
    return lower if (stack_size - lower) <= (upper - stack_size) else upper


def particle_number_of(eigs, mu, beta):
    """sum_s sum_k 1 / (1 + exp(beta (e_sk - mu)))."""
    x = beta * (numpy.asarray(eigs) - mu)
    return float(numpy.sum(0.5 * (1.0 - numpy.tanh(0.5 * x))))


def find_chemical_potential(eigs, beta, target, deps=1e-6, max_it=1000):
    mu1, mu2 = -1.0, 1.0
    while True:
        d1 = particle_number_of(eigs, mu1, beta) - target
        d2 = particle_number_of(eigs, mu2, beta) - target
        if numpy.sign(d1) * numpy.sign(d2) < 0:
            break
        mu1 -= 2
        mu2 += 2
    for _ in range(max_it):
        mu = 0.5 * (mu1 + mu2)
        d = particle_number_of(eigs, mu, beta) - target
        if abs(d) < deps:
            return mu
        if d * d1 > 0:
            mu1 = mu
        elif d * d2 > 0:
            mu2 = mu
    return None


class OneBody(object):

    def __init__(self, system, beta, dt, options={}, nav=None, H1=None, verbose=False):
        self.name = 'thermal'
        self.verbose = verbose
        if getattr(system, '_alt_convention', False):
            raise NotImplementedError("OneBody: the alternate sign convention of the chemical potential")
        self.H1 = numpy.asarray(system.H1 if H1 is None else H1)
        if numpy.iscomplexobj(self.H1) and numpy.any(self.H1.imag != 0):
            raise NotImplementedError("OneBody: a complex one-body Hamiltonian")
        self.H1 = numpy.ascontiguousarray(self.H1.real)
        dmat = numpy.array([scipy.linalg.expm(-dt * self.H1[0]), scipy.linalg.expm(-dt * self.H1[1])])
        self.nav = nav if nav is not None else options.get('nav', None)
        if self.nav is None:
            self.nav = system.nup + system.ndown
        self.max_it = options.get('max_it', 1000)
        self.deps = options.get('threshold', 1e-6)
        self.mu = options.get('mu', None)
        self.num_slices = int(beta / dt)
        self.stack_size = options.get('stack_size', None)
        self.cond = numpy.linalg.cond(dmat[0])
        if self.stack_size is None:
            # cond(BT)^stack_size <= 1e3 (onebody.py:56-71)
            self.stack_size = min(self.num_slices, int(3.0 / numpy.log10(self.cond)))
        self.stack_size = update_stack(self.stack_size, self.num_slices)
        self.num_bins = int(beta / (self.stack_size * dt))
        self.dtau = self.stack_size * dt
        eigs = numpy.array([scipy.linalg.eigvalsh(self.H1[0]), scipy.linalg.eigvalsh(self.H1[1])])
        tau = self.dtau * self.num_bins
        if self.mu is None:
            self.mu = find_chemical_potential(eigs, tau, self.nav, deps=self.deps, max_it=self.max_it)
            if self.mu is None:
                raise RuntimeError("OneBody: chemical potential not found")
        self.nav = particle_number_of(eigs, self.mu, tau)
        self.dmat = dmat * numpy.exp(dt * self.mu)
        self.dmat_inv = numpy.array([scipy.linalg.inv(self.dmat[0], check_finite=False),
                                     scipy.linalg.inv(self.dmat[1], check_finite=False)])
        self.error = False
        self.init = numpy.array([0])
