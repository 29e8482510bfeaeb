#!/usr/bin/env python3
"""Golden fixtures for generic Hamiltonians with COMPLEX Cholesky vectors, from the genuine reference.

Uses the import recipe and the recorders of make_golden.py (which it imports and does not change); runs only where
the reference is available.  Tests read the .npz files this writes.

  cplx_ops.npz   single-walker operations (Ghalf, G, force bias, VHS, phi after the exponential, the half-rotated and
                 the full-G local energies, one phaseless step on an equal-spin system) for a Hermitian complex L
                 (H_ prefix, L_n = (A_n + A_n^H) / 2) and a non-Hermitian one (N_ prefix)
  traj_cplx.npz  a short trajectory of the reference driver qmc/afqmc.py with Hermitian complex L
  msd_cplx.npz   a non-orthogonal multi-determinant trial (3 determinants) with Hermitian complex L: force bias, local
                 energy and ten phaseless steps of one walker (make_golden.py's msd_steps)

Usage:  python tests/golden/make_golden_cplx.py            (writes tests/golden/cplx_*.npz, traj_cplx.npz)
        python tests/golden/make_golden_cplx.py --check    regenerate into a scratch directory and compare
"""
import os
import shutil
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg                                                 # noqa: E402  (prepares the reference)
from make_golden import (Generic, MultiSlater, AFQMC, MPI, get_random_nomsd,   # noqa: E402
                         local_energy_generic_cholesky, single_walker_ops, record_trajectory, msd_steps, rand_phi)


def cplx_chol(M, K, hermitian, seed):
    """[M*M, K] complex Cholesky vectors: L_n = (A_n + A_n^H) / 2 (Hermitian) or A_n, A_n complex Gaussian, scaled so
    that the two-body part stays of the order of a molecular one."""
    rng = numpy.random.RandomState(seed)
    A = (rng.normal(size=(K, M, M)) + 1j * rng.normal(size=(K, M, M))) * (0.3 / numpy.sqrt(M))
    L = 0.5 * (A + A.conj().transpose(0, 2, 1)) if hermitian else A
    return numpy.ascontiguousarray(L.reshape(K, M * M).T)


def cplx_system(M, K, nelec, hermitian, seed):
    rng = numpy.random.RandomState(seed + 1)
    h = rng.normal(size=(M, M))
    h1e = 0.5 * (h + h.T) - 2.0 * numpy.eye(M)
    chol = cplx_chol(M, K, hermitian, seed)
    return Generic(nelec=nelec, h1e=numpy.array([h1e, h1e]), chol=chol, ecore=0.3), h1e, chol


def ops_case(out, tag, M, K, nelec, hermitian, seed):
    system, h1e, chol = cplx_system(M, K, nelec, hermitian, seed)
    numpy.random.seed(seed)
    wfn = get_random_nomsd(system, ndet=1, cplx=True)       # UHF-like: independent complex orbitals per spin
    trial = MultiSlater(system, wfn)
    trial.half_rotate(system)
    out[tag + 'h1e'] = h1e
    out[tag + 'chol'] = chol
    out[tag + 'ecore'] = 0.3
    out[tag + 'nelec'] = numpy.array(nelec)
    out[tag + 'h1e_mod'] = system.h1e_mod
    out[tag + 'rchol'] = trial._rchol
    trial.psi = trial.psi[0]
    single_walker_ops(system, trial, {}, 0.005, out, tag)
    # full-G energy of the walker's G (estimators/generic.py:398-434)
    out[tag + 'energy_full'] = numpy.array(local_energy_generic_cholesky(system, out[tag + 'G']))


def make_cplx_ops():
    out = {}
    ops_case(out, 'H_', 14, 30, (4, 3), True, 11)          # Hermitian, open shell
    ops_case(out, 'E_', 12, 24, (3, 3), True, 12)          # Hermitian, equal spins: the full phaseless step too
    ops_case(out, 'N_', 12, 24, (3, 3), False, 13)         # general complex L
    mg.save('cplx_ops.npz', out)


def make_traj_cplx():
    nmo, nelec = 11, (3, 3)
    options = {'verbosity': 0, 'get_sha1': False,
               'qmc': {'timestep': 0.005, 'steps': 5, 'blocks': 3, 'rng_seed': 8, 'nwalkers': 6,
                       'npop_control': 5},
               'estimates': {'mixed': {'energy_eval_freq': 1}},
               'trial': {'name': 'MultiSlater'}}
    system, h1e, chol = cplx_system(nmo, 25, nelec, True, 21)
    numpy.random.seed(7)
    comm = MPI.COMM_WORLD
    afqmc = AFQMC(comm=comm, system=system, options=options)
    # (systems/generic.py:209-210 stores h1e - v0 into a real array: the reference's one-body operator keeps only the
    #  real part of v0, which is complex for complex L; recorded so that a replay can use the same operator)
    out = {'h1e': h1e, 'chol': chol, 'ecore': 0.3, 'rchol': afqmc.trial._rchol, 'h1e_mod': system.h1e_mod}
    record_trajectory(afqmc, comm, out)
    assert len(out['parent_ix']) > 0
    mg.save('traj_cplx.npz', out)


def make_msd_cplx():
    out = {}
    nmo, nelec = 10, (4, 4)
    system, h1e, chol = cplx_system(nmo, 20, nelec, True, 31)
    out.update({'h1e': h1e, 'chol': chol, 'ecore': 0.3, 'nelec': numpy.array(nelec), 'h1e_mod': system.h1e_mod})
    numpy.random.seed(31)
    coeffs, wfn = get_random_nomsd(system, ndet=3, cplx=True)
    e, v = numpy.linalg.eigh(h1e)
    ref = numpy.concatenate([v[:, :4], v[:, :4]], axis=1)
    wfn = ref[None] + 0.15 * wfn
    init = ref + 0.1 * rand_phi(nmo, 8)
    trial = MultiSlater(system, (coeffs, wfn), init=init)
    msd_steps(system, trial, True, out, 'N_', eshift=0.3)
    mg.save('msd_cplx.npz', out)


FIXTURES = [('cplx_ops.npz', make_cplx_ops), ('traj_cplx.npz', make_traj_cplx), ('msd_cplx.npz', make_msd_cplx)]

if __name__ == '__main__':
    check = '--check' in sys.argv[1:]
    if check:
        import tempfile
        mg.OUT = tempfile.mkdtemp(prefix='golden_check_')
    failed = 0
    for name, make in FIXTURES:
        make()
        if check:
            bad = mg.compare_fixture(name, mg.OUT)
            print('%-20s %s' % (name, 'identical to the committed fixture' if not bad else 'DIFFERS: ' + '; '.join(bad[:6])))
            failed += bool(bad)
        else:
            print('%-20s %d bytes' % (name, os.path.getsize(os.path.join(mg.OUT, name))))
    if check:
        shutil.rmtree(mg.OUT, ignore_errors=True)
        sys.exit(1 if failed else 0)
