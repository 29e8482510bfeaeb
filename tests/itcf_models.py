"""Model builders of the ITCF GPU tests and of tools/itcf_bench.py: a Generic system with its device handle inputs,
and a device handle with the discrete Hirsch propagator on a Hubbard lattice."""
import numpy
import scipy.linalg

from pauxy_amd import _lib as L, systems, trial as trial_mod
from pauxy_amd.device import AfqDevice
from pauxy_amd.propagation import setup
from oracle import afqmc_ref as ref


def generic_model(M, K, na, nb, seed=3, dt=0.01, hermitian=False):
    """A Generic system with symmetric real (or, hermitian=True, Hermitian complex) Cholesky vectors, its trial and
    propagator arrays."""
    rng = numpy.random.RandomState(seed)
    h = rng.normal(size=(M, M))
    h1e = 0.5 * (h + h.T) - 2.0 * numpy.eye(M)
    A = rng.normal(size=(K, M, M)) * (0.3 / numpy.sqrt(M))
    if hermitian:
        A = A + 1j * rng.normal(size=(K, M, M)) * (0.3 / numpy.sqrt(M))
        Lv = 0.5 * (A + A.conj().transpose(0, 2, 1))
    else:
        Lv = 0.5 * (A + A.transpose(0, 2, 1))
    chol = numpy.ascontiguousarray(Lv.reshape(K, M * M).T)
    s = systems.Generic((na, nb), numpy.array([h1e, h1e]), chol, ecore=0.1)
    e, v = numpy.linalg.eigh(h1e)
    psi = numpy.zeros((M, na + nb), dtype=complex)
    psi[:, :na] = v[:, :na]
    psi[:, na:] = v[:, :nb]
    psi = psi + 0.05 * (rng.rand(M, na + nb) + 1j * rng.rand(M, na + nb))
    t = trial_mod.SingleDetTrial(s, psi)
    BH1, mf = setup.generic_propagator_arrays(s, t, dt)
    model = ref.RefModel('generic', M, na, nb, t.psi, BH1, mf, dt, hs_pot=s.hs_pot, rchol=t._rchol,
                         H1=s.H1.astype(complex), ecore=0.1)
    return model, s, rng


def hirsch_device(nx, ny, na, nb, nw, U=4.0, dt=0.05, seed=4):
    """A device with the discrete Hirsch propagator on an nx x ny Hubbard model and nw perturbed trial walkers."""
    s = systems.Hubbard(nx, ny, na, nb, U)
    M = nx * ny
    T = numpy.asarray(s.T, dtype=complex)
    BT2 = numpy.array([scipy.linalg.expm(-0.5 * dt * T[i]) for i in range(2)])
    e, v = numpy.linalg.eigh(T[0].real)
    rng = numpy.random.RandomState(seed)
    psi = numpy.hstack([v[:, :na], v[:, :nb]]).astype(complex)
    dev = AfqDevice(0)
    dev.set_system_hubbard(T, U, na, nb)
    dev.set_trial(psi)
    dev.set_propagator_hirsch(BT2, dt)
    dev.walkers_alloc(nw)
    ne = na + nb
    dev.set(L.F_PHI, numpy.array([psi + 0.05 * rng.rand(M, ne) for _ in range(nw)]))
    dev.set(L.F_OT, dev.calc_overlap())
    return dev, BT2, psi, rng, U, dt
