"""Continuous-field propagator of the finite-temperature algorithm for the Hubbard model, on the device.

Mirrors pauxy/thermal_propagation/continuous.py:14-120,202-257 (``Continuous``) with the Hubbard part of
thermal_propagation/hubbard.py:199-250 (``HubbardContinuous``, the charge form: v_i = n_iup + n_idown): the same
constructor signature -- ``(options, qmc, system, trial, verbose, lowrank)``, which is not ``PlaneWave``'s -- and
attributes, and ``propagate_walker(system, walker, trial, eshift)``.  Phaseless path with the force bias and the hybrid
weight, full-rank walkers, the degree-6 exponential: what the library's afq_thermal_propagate_continuous does on a
handle configured by afq_thermal_configure_hubbard_continuous.  The trial's density matrix and ``BH1`` are dense and
real; the field exponential is a diagonal.

Batched execution with the reference's random stream, as ``PlaneWave``: the reference draws
``numpy.random.normal(0, 1, nfields)`` once per walker, whatever the walker's weight; the first ``propagate_walker``
call of a time slice draws the fields of every walker in walker order and moves the whole population through the slice
with one call of the library; the calls for the other walkers of the slice return at once.
"""
import cmath

import numpy
import scipy.linalg

from pauxy_amd.propagation.thermal_planewave import BatchedFields


def left_table(BT, BT_inv, stack_size):
    """(BT^stack_size [2, M, M], left_k [stack_size, 2, M, M]) as the library builds them on the host for the slice
    kernel (afq_thermal_left_table): the reference's ``left`` after set_all and k + 1 slices of a bin."""
    from pauxy_amd import _lib
    BT = numpy.ascontiguousarray(numpy.real(BT), dtype=numpy.float64)
    BT_inv = numpy.ascontiguousarray(numpy.real(BT_inv), dtype=numpy.float64)
    M = BT.shape[-1]
    assert BT.shape == (2, M, M) and BT_inv.shape == (2, M, M)
    pw = numpy.empty((2, M, M))
    left = numpy.empty((int(stack_size), 2, M, M))
    rc = _lib.load().afq_thermal_left_table(M, int(stack_size), BT.ctypes.data, BT_inv.ctypes.data, pw.ctypes.data,
                                            left.ctypes.data)
    if rc:
        raise ValueError("afq_thermal_left_table: error %d" % rc)
    return pw, left


class HubbardContinuous(object):
    """hubbard.py:199-250: ``mf_shift``, ``mf_core``, ``iu_fac`` and the mean-field shifted ``BH1``."""

    def __init__(self, system, trial, qmc, options={}, verbose=False):
        if getattr(system, 'symmetric', False):
            raise NotImplementedError("Continuous (thermal): the symmetric form of the interaction")
        if getattr(system, '_alt_convention', False):
            raise NotImplementedError("Continuous (thermal): the alternate sign convention of the chemical potential")
        if getattr(system, 'mu', None) is None:
            raise ValueError("Continuous (thermal): the system needs a chemical potential (model: {mu: ...})")
        self.hs_type = 'hubbard_continuous'
        self.free_projection = False
        self.nstblz = qmc.nstblz
        self.dt = qmc.dt
        self.iu_fac = 1j * system.U ** 0.5
        self.sqrt_dt = qmc.dt ** 0.5
        self.isqrt_dt = 1j * self.sqrt_dt
        M = system.nbasis
        eye = numpy.identity(M)
        # trial.G of the reference: the Green's function of ONE slice, [I + dmat]^-1 (onebody.py:111); P = I - G^T
        P = numpy.array([eye - scipy.linalg.inv(eye + trial.dmat[s]).T for s in range(2)])
        self.mf_shift = self.construct_mean_field_shift(system, P)
        self.mf_core = 0.5 * numpy.dot(self.mf_shift, self.mf_shift)
        self.BH1 = None

    def construct_mean_field_shift(self, system, P):
        return self.iu_fac * (numpy.diag(P[0]) + numpy.diag(P[1]))

    def construct_one_body_propagator(self, system, dt):
        vi1b = self.iu_fac * numpy.diag(self.mf_shift)
        I = numpy.identity(system.nbasis, dtype=numpy.asarray(system.H1).dtype)
        muN = system.mu * I
        sign = -1                                   # (the alternate convention is refused above)
        H1 = system.h1e_mod - numpy.array([vi1b - sign * muN, vi1b - sign * muN])
        BH1 = numpy.array([scipy.linalg.expm(-0.5 * dt * H1[0]), scipy.linalg.expm(-0.5 * dt * H1[1])])
        if numpy.max(numpy.abs(BH1.imag)) != 0.0:
            raise NotImplementedError("Continuous (thermal): BH1 has a non-zero imaginary part (a real one-body "
                                      "propagator only)")
        self.BH1 = numpy.ascontiguousarray(BH1.real)


class Continuous(BatchedFields):
    def __init__(self, options, qmc, system, trial, verbose=False, lowrank=False):
        if system.name != "Hubbard":
            raise NotImplementedError("Continuous (thermal): Hubbard systems only (no Generic: the reference's thermal "
                                      "GenericContinuous cannot be reached; the UEG has PlaneWave)")
        if getattr(trial, 'name', '') != 'thermal' or not hasattr(trial, 'dmat_inv'):
            raise NotImplementedError("Continuous (thermal): a OneBody trial density matrix is needed (no MeanField)")
        if options.get('free_projection', False):
            raise NotImplementedError("Continuous (thermal): free_projection is not supported (phaseless path only)")
        if not options.get('force_bias', True):
            raise NotImplementedError("Continuous (thermal): force_bias: False is not supported")
        if lowrank or options.get('low_rank', False):
            raise NotImplementedError("Continuous (thermal): low_rank walkers are not supported")
        self.verbose = verbose
        self.hs_type = 'continuous'
        self.exp_nmax = options.get('expansion_order', 6)
        if self.exp_nmax != 6:
            raise NotImplementedError("Continuous (thermal): expansion_order %r is not supported (6 only)" % self.exp_nmax)
        self.dt = qmc.dt
        self.sqrt_dt = qmc.dt ** 0.5
        self.isqrt_dt = 1j * self.sqrt_dt
        self.lowrank = False
        self.propagator = HubbardContinuous(system, trial, qmc, options=options, verbose=verbose)
        self.mu = system.mu
        self.propagator.construct_one_body_propagator(system, qmc.dt)
        self.BH1 = self.propagator.BH1
        self.mf_shift = self.propagator.mf_shift
        self.BT = trial.dmat
        self.BTinv = trial.dmat_inv
        self.BT_BP = None
        self.mf_const_fac = cmath.exp(-self.dt * self.propagator.mf_core)
        self.nstblz = qmc.nstblz
        self.ebound = (2.0 / self.dt) ** 0.5
        self.mean_local_energy = 0
        self.free_projection = False
        self.force_bias = True
        BatchedFields.__init__(self)

    @property
    def nfb_trig(self):
        """The number of force-bias components rescaled so far (continuous.py:104-110 counts them): the handle's
        counter (afq_counters [0]), which lives as long as the handle and counts for every propagator of that handle."""
        return 0 if self._dev is None else int(self._dev.counters()[0])
