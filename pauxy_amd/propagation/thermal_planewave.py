"""Plane-wave propagator of the finite-temperature algorithm for the uniform electron gas, on the device.

Mirrors pauxy/thermal_propagation/planewave.py:15-82,219-276,445-517 (``PlaneWave``): the same constructor signature and
attributes (``hs_type``, ``free_projection``, ``optimised``, ``exp_nmax``, ``fb_bound``, ``mf_shift`` built from the
trial's one-slice density matrix, ``BH1 = expm(-dt/2 h1e_mod + dt/2 mu)``, ``BT``, ``BTinv``, ``mf_const_fac``,
``nfb_trig``) and ``propagate_walker(system, walker, trial, eshift)``.  Phaseless (constrained) path with the force bias,
full-rank walkers, the degree-6 exponential: what the library's afq_thermal_propagate_continuous does.  ``optimised``
is accepted either way: the reference's left / right form and its plain form compute the same Green's function
G = [I + bin[nbins - 1] .. bin[0]]^-1, which is what the device evaluates.

Batched execution with the reference's random stream: the reference draws ``numpy.random.normal(0, 1, nfields)`` once
per walker, whatever the walker's weight (the thermal driver skips no walker); the first ``propagate_walker`` call of a
time slice draws the fields of every walker in walker order and moves the whole population through the slice with one
call of the library; the calls for the other walkers of the slice return at once.  The driver hands the time slice
where the propagator expects the trial, and 0 for ``eshift``: neither is used.
"""
import numpy
import scipy.linalg

from pauxy_amd.context import hidden


def planewave_constants(system, trial, dt):
    """(BH1 [2, M, M], mf_shift [nfields]) of planewave.py:83-108."""
    if getattr(system, 'mu', None) is None:
        raise ValueError("PlaneWave (thermal): the system needs a chemical potential (model: {mu: ...})")
    M = system.nbasis
    eye = numpy.identity(M)
    H1 = numpy.asarray(system.h1e_mod).real
    BH1 = numpy.array([scipy.linalg.expm(-0.5 * dt * H1[0] + 0.5 * dt * system.mu * eye),
                       scipy.linalg.expm(-0.5 * dt * H1[1] + 0.5 * dt * system.mu * eye)])
    # trial.G of the reference: the Green's function of ONE slice, [I + dmat]^-1 (onebody.py:111); P = I - G^T
    P = numpy.array([eye - scipy.linalg.inv(eye + trial.dmat[s]).T for s in range(2)]).reshape(2, M * M)
    nq = system.nfields // 2
    mf_shift = numpy.zeros(system.nfields, dtype=numpy.complex128)
    mf_shift[:nq] = system.iA.T.dot(P[0]) + system.iA.T.dot(P[1])
    mf_shift[nq:] = system.iB.T.dot(P[0]) + system.iB.T.dot(P[1])
    return BH1, mf_shift


class BatchedFields(object):
    """What the propagators with continuous fields share (``PlaneWave`` here, ``Continuous`` for the Hubbard model): one
    call of the library per time slice for the whole population, behind the reference's per-walker interface."""
    _pending = hidden()         # calls of the current slice still to swallow, per population
    _dev = hidden()             # the device of the population moved last: its counters are behind nfb_trig

    def __init__(self):
        self._pending = {}
        self._dev = None
        self.last_fields = None

    def propagate_walkers(self, walk, eshift=0):
        """One time slice of the whole population (planewave.py:445-517, continuous.py:202-257 for every walker)."""
        walk.ensure_configured(self)
        dev = self._dev = walk.dev
        xi = numpy.empty((dev.nw, dev.K))
        for iw in range(dev.nw):
            xi[iw] = numpy.random.normal(0.0, 1.0, dev.K)                 # planewave.py:240, continuous.py:97
        dev.thermal_propagate_continuous(xi)
        self.last_fields = xi
        walk.time_slice += 1

    def propagate_walker(self, system, walker, trial, eshift=0):
        walk = walker._h
        left = self._pending.get(id(walk), 0)
        if left > 0:
            self._pending[id(walk)] = left - 1
            return
        self.propagate_walkers(walk, eshift)
        self._pending[id(walk)] = walk.nw - 1             # (set behind the call: a slice that raised leaves nothing to swallow)

    propagate_walker_phaseless = propagate_walker


class PlaneWave(BatchedFields):
    def __init__(self, system, trial, qmc, options={}, verbose=False, lowrank=False):
        if system.name != "UEG":
            raise NotImplementedError("PlaneWave (thermal): UEG systems only (no Generic, no continuous Hubbard)")
        if getattr(trial, 'name', '') != 'thermal' or not hasattr(trial, 'dmat_inv'):
            raise NotImplementedError("PlaneWave (thermal): a OneBody trial density matrix is needed (no MeanField)")
        if options.get('free_projection', False):
            raise NotImplementedError("PlaneWave (thermal): free_projection is not supported (constrained path only)")
        if lowrank:
            raise NotImplementedError("PlaneWave (thermal): low_rank walkers are not supported")
        self.verbose = verbose
        self.hs_type = 'plane_wave'
        self.free_projection = False
        self.optimised = options.get('optimised', True)
        self.lowrank = False
        self.exp_nmax = options.get('expansion_order', 6)
        if self.exp_nmax != 6:
            raise NotImplementedError("PlaneWave (thermal): expansion_order %r is not supported (6 only)" % self.exp_nmax)
        self.nstblz = qmc.nstblz
        self.fb_bound = float(options.get('fb_bound', 1.0))
        self.dt = qmc.dt
        self.sqrt_dt = qmc.dt ** 0.5
        self.isqrt_dt = 1j * self.sqrt_dt
        self.num_vplus = system.nfields // 2
        self.BH1, self.mf_shift = planewave_constants(system, trial, qmc.dt)
        self.BT = trial.dmat
        self.BTinv = trial.dmat_inv
        self.mf_const_fac = 1
        self.BT_BP = self.BT
        self.ebound = (2.0 / self.dt) ** 0.5
        self.mean_local_energy = 0
        BatchedFields.__init__(self)

    @property
    def nfb_trig(self):
        """False until a component of the force bias was rescaled, True from then on, across resets and paths, as the
        reference's flag ("printed once per thread").  It reads the handle's count of rescaled force-bias components
        (afq_counters [0]), which lives as long as the handle and counts for every propagator of that handle."""
        return self._dev is not None and int(self._dev.counters()[0]) > 0
