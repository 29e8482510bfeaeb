#!/usr/bin/env python3
"""Golden fixture for the back-propagation window of a multi-determinant trial, from the genuine reference.

The reference's BackPropagation cannot run with ndets > 1 (DESIGN row 8f-2), so this fixture pins the per-determinant
pieces of the specification that tests/bp_msd_ref.py restates: the genuine back_propagate_generic applied to every
determinant D_d of a 3-determinant trial over field histories, composed with the genuine gab.  The histories are never
re-orthogonalised (nstblz > nbp): without a re-orthogonalisation the reference's per-determinant pieces compose exactly
(log r_d = 0), so the backward pass, the Green's functions and the weights are all the reference's own.

  bp_msd.npz   system (M = 8, 3+2, real symmetric vectors), BT2, dt; 3 complex determinants and coefficients; per
               walker (3 of them): fields [nbp, K], phi_old; per (walker, d): the back-propagated determinant,
               G_d = gab(D_d^bp, phi_old)^T per spin and <D_d^bp|phi_old>

Uses the import recipe of make_golden.py (which it imports and does not change); runs only where the reference is
available.

Usage:  python tests/golden/make_golden_bp_msd.py            (writes tests/golden/bp_msd.npz)
        python tests/golden/make_golden_bp_msd.py --check    regenerate into a scratch directory and compare
"""
import os
import shutil
import sys

import numpy
import scipy.linalg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg                                                 # noqa: E402  (prepares the reference)
from make_golden import Generic, generate_hamiltonian                    # noqa: E402
from pauxy.estimators.greens_function import gab                        # noqa: E402
from pauxy.propagation.generic import back_propagate_generic            # noqa: E402


class _Configs(object):
    """What back_propagate_generic reads of a FieldConfig: get_block()[0], the recorded fields oldest first."""
    def __init__(self, configs):
        self.configs = configs

    def get_block(self):
        return (self.configs,)


def make():
    out = {}
    rng = numpy.random.RandomState(23)
    numpy.random.seed(9)
    nmo, nelec, dt = 8, (3, 2), 0.01
    na = nelec[0]
    h1e, chol, enuc, eri = generate_hamiltonian(nmo, nelec, cplx=False)
    system = Generic(nelec=nelec, h1e=numpy.array([h1e, h1e]), chol=chol.reshape((-1, nmo * nmo)).T.copy(), ecore=enuc)
    BT2 = numpy.array([scipy.linalg.expm(-0.5 * dt * h1e)] * 2)
    K = system.chol_vecs.shape[1]
    nbp, nstblz, nw, nd = 5, 7, 3, 3
    e, v = numpy.linalg.eigh(h1e)
    base = numpy.hstack([v[:, :nelec[0]], v[:, :nelec[1]]]).astype(complex)
    dets = numpy.array([base + 0.1 * (rng.rand(nmo, sum(nelec)) + 1j * rng.rand(nmo, sum(nelec))) for _ in range(nd)])
    coeffs = numpy.array([0.8 + 0.1j, 0.4 - 0.3j, -0.2 + 0.25j])
    fields = rng.normal(size=(nw, nbp, K)) + 0.3j * rng.normal(size=(nw, nbp, K))
    phi_old = numpy.array([base + 0.1 * (rng.rand(nmo, sum(nelec)) + 1j * rng.rand(nmo, sum(nelec))) for _ in range(nw)])
    bp = numpy.zeros((nw, nd, nmo, sum(nelec)), dtype=complex)
    G = numpy.zeros((nw, nd, 2, nmo, nmo), dtype=complex)
    ov = numpy.zeros((nw, nd), dtype=complex)
    for w in range(nw):
        for d in range(nd):
            phi = dets[d].copy()                             # (propagated in place)
            back_propagate_generic(phi, _Configs(fields[w]), system, nstblz, BT2, dt)
            bp[w, d] = phi
            G[w, d, 0] = gab(phi[:, :na], phi_old[w][:, :na]).T
            G[w, d, 1] = gab(phi[:, na:], phi_old[w][:, na:]).T
            ov[w, d] = (scipy.linalg.det(phi[:, :na].conj().T.dot(phi_old[w][:, :na])) *
                        scipy.linalg.det(phi[:, na:].conj().T.dot(phi_old[w][:, na:])))
    out.update(hs_pot=system.chol_vecs, BT2=BT2, dt=dt, nelec=numpy.array(nelec), nstblz=nstblz, dets=dets,
               coeffs=coeffs, fields=fields, phi_old=phi_old, bp=bp, G=G, ovlp=ov)
    mg.save('bp_msd.npz', out)


if __name__ == '__main__':
    check = '--check' in sys.argv[1:]
    if check:
        import tempfile
        mg.OUT = tempfile.mkdtemp(prefix='golden_check_')
    make()
    if check:
        bad = mg.compare_fixture('bp_msd.npz', mg.OUT)
        print('bp_msd.npz %s' % ('identical to the committed fixture' if not bad else 'DIFFERS: ' + '; '.join(bad[:6])))
        shutil.rmtree(mg.OUT, ignore_errors=True)
        sys.exit(1 if bad else 0)
    print('bp_msd.npz %d bytes' % os.path.getsize(os.path.join(mg.OUT, 'bp_msd.npz')))
