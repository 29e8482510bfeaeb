"""Discrete Hirsch propagator of the finite-temperature algorithm for the Hubbard model, on the device.

Mirrors pauxy/thermal_propagation/hubbard.py:8-142 (``ThermalDiscrete``): the same constructor signature and constants
(``gamma``, ``auxf`` with the chemical-potential shift ``dmu = -(system.mu - trial.mu)`` folded in, ``delta``, ``BH1 =
expm(-dt (H1 - mu I))``, ``BT``, ``BT_inv``, ``nstblz``, ``hs_type``) and ``propagate_walker(system, walker, time_slice,
eshift)``.  Spin decomposition and the constrained path only: every matrix is real.

Batched execution with the reference's random stream: the reference draws ``numpy.random.random()`` once per site and
walker, whatever the walker's weight; the first ``propagate_walker`` call of a time slice draws the M uniforms of every
walker in walker order and moves the whole population through the slice with one call of the library
(afq_thermal_propagate: site updates, stack update, refresh, wrap); the calls for the other walkers of the slice
return at once.
"""
import numpy
import scipy.linalg

from pauxy_amd.context import hidden


def thermal_constants(system, trial, dt):
    """(auxf [field, spin], BH1 [2, M, M], mu used in BH1) of hubbard.py:15-66."""
    if getattr(system, 'symmetric', False):
        raise NotImplementedError("ThermalDiscrete: the symmetric form of the interaction")
    if getattr(system, '_alt_convention', False):
        raise NotImplementedError("ThermalDiscrete: the alternate sign convention of the chemical potential")
    gamma = numpy.arccosh(numpy.exp(0.5 * dt * system.U))
    auxf = numpy.array([[numpy.exp(gamma), numpy.exp(-gamma)], [numpy.exp(-gamma), numpy.exp(gamma)]])
    auxf = auxf * numpy.exp(-0.5 * dt * system.U)
    dmu = -(system.mu - trial.mu)
    auxf = auxf * numpy.exp(-dt * dmu)
    mu = trial.mu if abs(dmu) > 1e-16 else system.mu
    H1 = numpy.asarray(system.H1).real
    eye = numpy.identity(H1.shape[-1])
    BH1 = numpy.array([scipy.linalg.expm(-dt * (H1[0] - mu * eye)), scipy.linalg.expm(-dt * (H1[1] - mu * eye))])
    return gamma, auxf, dmu, mu, BH1


class ThermalDiscrete(object):
    _slice_done = hidden()          # (population, time slice) the batched call has already moved

    def __init__(self, system, trial, qmc, options={}, verbose=False, lowrank=False):
        if system.name != "Hubbard":
            raise NotImplementedError("ThermalDiscrete: Hubbard systems only (no Generic / UEG)")
        if getattr(trial, 'name', '') != 'thermal' or not hasattr(trial, 'dmat_inv'):
            raise NotImplementedError("ThermalDiscrete: a OneBody trial density matrix is needed (no MeanField)")
        if options.get('charge_decomposition', False):
            raise NotImplementedError("ThermalDiscrete: charge_decomposition is not supported (spin decomposition only)")
        if options.get('free_projection', False):
            raise NotImplementedError("ThermalDiscrete: free_projection is not supported (constrained path only)")
        if lowrank:
            raise NotImplementedError("ThermalDiscrete: low_rank walkers are not supported")
        self.free_projection = False
        self.nstblz = qmc.nstblz
        self.hs_type = 'discrete'
        self.charge_decomp = False
        self.gamma, self.auxf, self.dmu, self._mu, self.BH1 = thermal_constants(system, trial, qmc.dt)
        self.aux_wfac = numpy.array([1.0, 1.0])
        self.delta = self.auxf - 1
        self.BT_BP = None
        self.BT = trial.dmat
        self.BT_inv = trial.dmat_inv
        self.hybrid = False
        self._slice_done = None
        self.last_fields = None

    def propagate_walkers(self, walk, eshift=0):
        """One time slice of the whole population (hubbard.py:117-142 for every walker)."""
        walk.ensure_configured(self)
        dev = walk.dev
        u = numpy.empty((dev.nw, dev.M))
        for iw in range(dev.nw):
            for i in range(dev.M):
                u[iw, i] = numpy.random.random()                       # hubbard.py:122
        self.last_fields = dev.thermal_propagate(u, eshift, fetch_fields=True)
        walk.time_slice += 1

    def propagate_walker(self, system, walker, time_slice, eshift=0):
        walk = walker._h
        key = (id(walk), walk.path_index, time_slice)
        if self._slice_done == key:
            return
        self._slice_done = key
        self.propagate_walkers(walk, eshift)

    propagate_walker_constrained = propagate_walker
