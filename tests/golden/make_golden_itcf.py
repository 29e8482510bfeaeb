#!/usr/bin/env python3
"""Golden fixtures for the imaginary-time Green's function (ITCF), from the genuine reference.

The reference's own ITCF estimator cannot run (DESIGN row 8f-3), so these fixtures pin the building blocks of the
specification that tests/itcf_ref.py restates, and the window semantics it shares with the back-propagated estimator:

  itcf_blocks.npz   construct_propagator_matrix_generic and the discrete Hubbard construct_propagator_matrix (with dt)
                    on field histories; back_propagate_generic(..., store=True); gab; reortho
  itcf_windows.npz  one recorded driver window of a small Generic run (11 orbitals, 3+3, restore_weights 'full') and of
                    the 4x4 Hirsch run (7+7): every walker's fields, weight, cosine / phase factors and phi_old (psi_R(0)),
                    the trial, BT2, and the back-propagated estimator's sums of that window (denominator, sum_w wt_w G_bp^T)

Uses the import recipe of make_golden.py (which it imports and does not change); runs only where the reference is
available.

Usage:  python tests/golden/make_golden_itcf.py            (writes tests/golden/itcf_*.npz)
        python tests/golden/make_golden_itcf.py --check    regenerate into a scratch directory and compare
"""
import os
import shutil
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg                                                 # noqa: E402  (prepares the reference)
from make_golden import Generic, Hubbard, generate_hamiltonian          # noqa: E402
import pauxy.estimators.back_propagation as ref_bp                       # noqa: E402
from pauxy.estimators.greens_function import gab                        # noqa: E402
from pauxy.propagation.generic import (                                  # noqa: E402
    construct_propagator_matrix_generic, back_propagate_generic)
from pauxy.propagation.hubbard import construct_propagator_matrix       # noqa: E402
from pauxy.utils.linalg import reortho                                   # noqa: E402


class _Configs(object):
    """What back_propagate_generic reads of a FieldConfig: get_block()[0], the recorded fields oldest first."""
    def __init__(self, configs):
        self.configs = configs

    def get_block(self):
        return (self.configs,)


def make_blocks():
    out = {}
    rng = numpy.random.RandomState(11)
    numpy.random.seed(5)
    nmo, nelec, dt = 8, (3, 2), 0.01
    h1e, chol, enuc, eri = generate_hamiltonian(nmo, nelec, cplx=False)
    system = Generic(nelec=nelec, h1e=numpy.array([h1e, h1e]), chol=chol.reshape((-1, nmo * nmo)).T.copy(), ecore=enuc)
    import scipy.linalg
    BT2 = numpy.array([scipy.linalg.expm(-0.5 * dt * h1e)] * 2)
    K = system.chol_vecs.shape[1]
    n = 7
    x = rng.normal(size=(n, K)) + 0.3j * rng.normal(size=(n, K))
    out['g_hs_pot'] = system.chol_vecs
    out['g_BT2'] = BT2
    out['g_dt'] = dt
    out['g_nelec'] = numpy.array(nelec)
    out['g_fields'] = x
    out['g_B'] = numpy.array([construct_propagator_matrix_generic(system, BT2, c, dt) for c in x])
    phi = rng.rand(nmo, sum(nelec)) + 1j * rng.rand(nmo, sum(nelec))
    out['g_bp_phi'] = phi.copy()
    out['g_bp_nstblz'] = 3
    out['g_bp_store'] = numpy.array(back_propagate_generic(phi.copy(), _Configs(x), system, 3, BT2, dt, store=True))
    hub = Hubbard({'name': 'Hubbard', 'nx': 4, 'ny': 4, 'nup': 7, 'ndown': 7, 'U': 4.0}, verbose=False)
    M = 16
    dth = 0.05
    bt2 = numpy.array([scipy.linalg.expm(-0.5 * dth * hub.T[0]), scipy.linalg.expm(-0.5 * dth * hub.T[1])])
    xh = rng.randint(0, 2, size=(4, M)).astype(numpy.complex128)
    out['h_T'] = numpy.array(hub.T)
    out['h_U'] = hub.U
    out['h_dt'] = dth
    out['h_BT2'] = bt2
    out['h_fields'] = xh
    out['h_B'] = numpy.array([construct_propagator_matrix(hub, bt2, c, dth) for c in xh])
    A = rng.rand(10, 4) + 1j * rng.rand(10, 4)
    B = rng.rand(10, 4) + 1j * rng.rand(10, 4)
    out['gab_A'], out['gab_B'] = A, B
    out['gab'] = gab(A, B)
    Q, detR = reortho(A.copy())
    out['reortho_in'] = A
    out['reortho_Q'] = Q
    out['reortho_detR'] = detR
    mg.save('itcf_blocks.npz', out)


# ---- one driver window, captured around the reference's own BackPropagation.update_uhf
_CAP = {}
_update_uhf = ref_bp.BackPropagation.update_uhf


def _cap_update_uhf(self, system, qmc, trial, psi, step, free_projection=False):
    buff_ix = psi.walkers[0].field_configs.step
    first = not _CAP.get('done') and buff_ix in self.splits
    if first:
        w = psi.walkers
        _CAP.update(
            fields=numpy.array([x.field_configs.get_block()[0].copy() for x in w]),
            weight=numpy.array([x.weight for x in w], dtype=numpy.float64),
            cos=numpy.array([x.field_configs.get_wfac()[0] for x in w], dtype=numpy.float64),
            ph=numpy.array([x.field_configs.get_wfac()[1] for x in w], dtype=numpy.complex128),
            phi_old=numpy.array([x.phi_old.copy() for x in w]),
            psi=numpy.array(trial.psi).copy(), BT2=numpy.array(self.BT2), dt=qmc.dt, nstblz=self.nstblz,
            restore=self.restore_weights or '', before=self.estimates.copy())
    try:
        return _update_uhf(self, system, qmc, trial, psi, step, free_projection)
    finally:
        if first:
            d = self.estimates - _CAP['before']
            M = self.G.shape[-1]
            _CAP.update(done=True, denom=d[self.nreg], G_sum=d[self.nreg + 1:self.nreg + 1 + 2 * M * M].reshape(2, M, M))
            if system.name == 'Generic':
                _CAP['hs_pot'] = numpy.array(system.chol_vecs)
            else:
                _CAP['U'] = system.U


ref_bp.BackPropagation.update_uhf = _cap_update_uhf


def _capture(run, tag, out):
    _CAP.clear()
    real_save = mg.save
    mg.save = lambda nm, o: None
    mg.h5py._STORE.clear()
    try:
        run()
    finally:
        mg.save = real_save
    assert _CAP.get('done'), tag
    for k in ('fields', 'weight', 'cos', 'ph', 'phi_old', 'psi', 'BT2', 'dt', 'nstblz', 'restore', 'denom', 'G_sum'):
        out[tag + k] = _CAP[k]
    for k in ('hs_pot', 'U'):
        if k in _CAP:
            out[tag + k] = _CAP[k]


def make_windows():
    out = {}
    _capture(lambda: mg.make_traj_bp('scratch.npz', restore_weights='full', blocks=1), 'g_', out)
    _capture(lambda: mg.make_traj_hirsch('scratch.npz', blocks=1, bp={'tau_bp': 0.04, 'one_rdm': True}), 'h_', out)
    mg.save('itcf_windows.npz', out)


FIXTURES = [
    ('itcf_blocks.npz', make_blocks),
    ('itcf_windows.npz', make_windows),
]


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if a != '--check']
    check = '--check' in sys.argv[1:]
    chosen = [f for f in FIXTURES if not args or f[0] in args]
    if check:
        import tempfile
        mg.OUT = tempfile.mkdtemp(prefix='golden_check_')
    failed = 0
    for name, make in chosen:
        make()
        if check:
            bad = mg.compare_fixture(name, mg.OUT)
            print('%-24s %s' % (name, 'identical to the committed fixture' if not bad else 'DIFFERS: ' + '; '.join(bad[:6])))
            failed += bool(bad)
        else:
            print('%-24s %d bytes' % (name, os.path.getsize(os.path.join(mg.OUT, name))))
    if check:
        shutil.rmtree(mg.OUT, ignore_errors=True)
        print('%d of %d fixtures differ' % (failed, len(chosen)) if failed else 'all %d fixtures reproduce' % len(chosen))
        sys.exit(1 if failed else 0)
