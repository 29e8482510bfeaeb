#!/usr/bin/env python3
"""Golden fixtures for the back-propagated two-body RDM and EKT Fock matrices, from the genuine reference.

Uses the import recipe and the recorders of make_golden.py (which it imports and does not change); runs only where
the reference is available.  Tests read the .npz files this writes.

  bp_obs_generic.npz  make_traj_bp's system (M = 11, 3+3, tau_bp = 5 steps) with two_rdm and evaluate_ekt
  bp_obs_split.npz    the same with nsplit = 2 (windows of 3 and 6 steps)
  bp_obs_ueg.npz      traj_bp_ueg's model (M = 33, nq = 256) with two_rdm and evaluate_ekt: the new outputs only,
                      the run itself is bitwise traj_bp_ueg.npz's (checked here)
  bp_obs_hirsch.npz   discrete Hirsch 4x4 Hubbard with two_rdm
  bp_obs_quirk.npz    one_rdm: False with evaluate_ekt: the reference's print_step slices the Fock matrices from the
                      region of the one-body RDM (back_propagation.py:309-313)
  bp_obs_direct.npz   ekt_1p_fock_opt / ekt_1h_fock_opt on random Green's functions, real and complex vectors

Generic systems store their vectors as [M*M, K], which ekt.py's `assert len(cholvec.shape) == 3` refuses: the
reference's EKT dies with an AssertionError there.  For those runs this script hands the reference's own functions
L_x[i, k] = chol[i*M + k, x], reshaped at run time (the layout the UEG branch of back_propagation.py builds).

Every window's Fock matrices are stored, and every walker's G_bp and weight of the first window (bp_win0_*).  The M^4 two-body RDMs are stored in full only while they stay small; every
window keeps the elements at a fixed set of flat indices (bp_two_rdm_idx).

Usage:  python tests/golden/make_golden_bp_obs.py            (writes tests/golden/bp_obs_*.npz)
        python tests/golden/make_golden_bp_obs.py --check    regenerate into a scratch directory and compare
"""
import os
import shutil
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg                                                 # noqa: E402  (prepares the reference)
from make_golden import Generic, AFQMC, MPI, generate_hamiltonian, record_trajectory   # noqa: E402
import pauxy.estimators.back_propagation as ref_bp                       # noqa: E402
from pauxy.estimators.ekt import ekt_1p_fock_opt, ekt_1h_fock_opt        # noqa: E402

NSAMP = 2048               # sampled two-body RDM elements per window
FULL_BYTES = 600 * 1024    # full two-body RDMs kept while they take at most this much


def _as3(cholvec):
    cholvec = numpy.asarray(cholvec)
    if cholvec.ndim == 2:                  # Generic: [M*M, K] -> L_x[i, k] = chol[i*M + k, x]
        M = int(round(numpy.sqrt(cholvec.shape[0])))
        cholvec = cholvec.T.reshape(cholvec.shape[1], M, M)
    return cholvec


def _ekt_1p(h1, cholvec, rdm1a, rdm1b):
    return ekt_1p_fock_opt(h1, _as3(cholvec), rdm1a, rdm1b)


def _ekt_1h(h1, cholvec, rdm1a, rdm1b):
    return ekt_1h_fock_opt(h1, _as3(cholvec), rdm1a, rdm1b)


ref_bp.ekt_1p_fock_opt = _ekt_1p
ref_bp.ekt_1h_fock_opt = _ekt_1h

# every walker's G_bp and weight of the first window a run evaluates (recorded around the reference's own update_uhf
# and gab), so that a window can be recomputed from them (bp_win0_*)
_CAP = {}
_update_uhf, _gab = ref_bp.BackPropagation.update_uhf, ref_bp.gab


def _cap_reset():
    _CAP.clear()
    _CAP.update(active=False, done=False, G=[], wt=[], split=0)


def _cap_update_uhf(self, system, qmc, trial, psi, step, free_projection=False):
    buff_ix = psi.walkers[0].field_configs.step
    first = not _CAP['done'] and buff_ix in self.splits
    if first:
        assert self.restore_weights is None                # the weight is then wnm.weight (back_propagation.py:199)
        _CAP.update(active=True, G=[], wt=[w.weight for w in psi.walkers], split=int(buff_ix))
    try:
        return _update_uhf(self, system, qmc, trial, psi, step, free_projection)
    finally:
        if first:
            _CAP.update(active=False, done=True)


def _cap_gab(A, B):
    g = _gab(A, B)
    if _CAP.get('active'):
        _CAP['G'].append(g.T.copy())
    return g


ref_bp.BackPropagation.update_uhf = _cap_update_uhf
ref_bp.gab = _cap_gab


def _cap_store(out, M):
    nw = len(_CAP['wt'])
    assert _CAP['done'] and len(_CAP['G']) == 2 * nw
    out['bp_win0_G'] = numpy.array(_CAP['G']).reshape(nw, 2, M, M)
    out['bp_win0_wt'] = numpy.array(_CAP['wt'], dtype=numpy.complex128)
    out['bp_win0_split'] = _CAP['split']


def _series(store, kind, sp):
    keys = sorted((k for k in store if k.startswith('back_propagated/%s_%d/' % (kind, sp))),
                  key=lambda k: int(k.rsplit('/', 1)[1]))
    return numpy.array([store[k] for k in keys])


def bp_outputs(store, splits, M, out):
    """Every back_propagated/<kind>_<split> series of the run's in-memory estimates file."""
    rng = numpy.random.RandomState(1234)
    idx = numpy.sort(rng.choice(M ** 4, size=min(NSAMP, M ** 4), replace=False)).astype(numpy.int64)
    for sp in splits:
        sfx = '' if len(splits) == 1 else '_%d' % sp
        den = _series(store, 'denominator', sp)
        assert len(den) > 0, sp
        out['bp_denominator' + sfx] = den.reshape(len(den))
        for kind in ('one_rdm', 'fock_1p', 'fock_1h'):
            s = _series(store, kind, sp)
            if len(s):
                assert len(s) == len(den), kind
                out['bp_' + kind + sfx] = s
        t = _series(store, 'two_rdm', sp)
        if len(t):
            assert len(t) == len(den) and t.shape[1:] == (M, M, M, M)
            out['bp_two_rdm_idx'] = idx
            out['bp_two_rdm_samp' + sfx] = t.reshape(len(t), -1)[:, idx]
            nfull = min(len(t), FULL_BYTES // (16 * M ** 4))
            if nfull:
                out['bp_two_rdm_full' + sfx] = t[:nfull]


def traj_generic(name, bp, blocks=2, tau_bp=0.025):
    """make_golden.make_traj_bp's run (qmc/tests/test_afqmc.py:232-278) with further back-propagation options."""
    out = {}
    nmo, nelec = 11, (3, 3)
    bp = dict(bp, tau_bp=tau_bp)
    options = {'verbosity': 0, 'get_sha1': False,
               'qmc': {'timestep': 0.005, 'num_steps': 10, 'blocks': blocks, 'rng_seed': 8},
               'trial': {'name': 'MultiSlater'},
               'estimator': {'back_propagated': bp, 'mixed': {'energy_eval_freq': 1}}}
    numpy.random.seed(7)
    h1e, chol, enuc, eri = generate_hamiltonian(nmo, nelec, cplx=False)
    system = Generic(nelec=nelec, h1e=numpy.array([h1e, h1e]),
                     chol=chol.reshape((-1, nmo * nmo)).T.copy(), ecore=enuc)
    comm = MPI.COMM_WORLD
    mg.h5py._STORE.clear()
    _cap_reset()
    afqmc = AFQMC(comm=comm, system=system, options=options)
    assert afqmc.estimators.back_propagation and afqmc.estimators.nbp == int(round(tau_bp / 0.005))
    out['h1e'] = h1e
    out['chol'] = system.chol_vecs
    out['ecore'] = enuc
    out['nbp'] = afqmc.estimators.nbp
    record_trajectory(afqmc, comm, out)
    est = afqmc.estimators.estimators['back_prop']
    splits = [int(x) for x in est.splits]
    out['splits'] = numpy.array(splits)
    bp_outputs(mg.h5py._STORE[afqmc.estimators.filename], splits, nmo, out)
    _cap_store(out, nmo)
    mg.save(name, out)


def _with_bp_options(extra):
    """An AFQMC constructor that adds ``extra`` to the back_propagated options of the input it is handed."""
    def make(*a, **k):
        opts = k.get('options')
        for sec in ('estimates', 'estimator', 'estimators'):
            if opts is not None and 'back_propagated' in opts.get(sec, {}):
                opts[sec]['back_propagated'].update(extra)
        return AFQMC(*a, **k)
    return make


def _rerun(make, name, M, base=None):
    """Runs one of make_golden's BP fixtures with the options patched in, then stores its new outputs too.  With
    ``base`` (a committed fixture of that same run) only what the base does not hold is stored, after checking that
    everything the base holds came out bitwise the same."""
    saved = {}
    real_save = mg.save
    mg.save = lambda nm, out: saved.update(out)
    mg.h5py._STORE.clear()
    _cap_reset()
    try:
        make()
    finally:
        mg.save = real_save
    stores = [s for s in mg.h5py._STORE.values() if any(k.startswith('back_propagated/') for k in s)]
    assert len(stores) == 1
    out = dict(saved)
    nbp = int(out['nbp'])
    bp_outputs(stores[0], [nbp], M, out)
    _cap_store(out, M)
    if base is not None:
        b = numpy.load(os.path.join(mg.HERE, base), allow_pickle=False)
        out['blocks'] = numpy.array(out['blocks'])
        out['blocks'][:, -1] = 0                      # the wall clock, zeroed by save() as well
        out['final_estimates'] = numpy.array(out['final_estimates'])
        out['final_estimates'][9] = 0
        for k in b.files:
            assert numpy.array_equal(b[k], out[k], equal_nan=b[k].dtype.kind in 'fc'), k
        out = {k: v for k, v in out.items() if k not in b.files}
    mg.save(name, out)


def make_ueg():
    real = mg.AFQMC
    mg.AFQMC = _with_bp_options({'two_rdm': True, 'evaluate_ekt': True})
    try:
        _rerun(lambda: mg.make_traj_bp_ueg('scratch.npz'), 'bp_obs_ueg.npz', 33, base='traj_bp_ueg.npz')
    finally:
        mg.AFQMC = real


def make_hirsch():
    _rerun(lambda: mg.make_traj_hirsch('scratch.npz', blocks=2,
                                       bp={'tau_bp': 0.04, 'one_rdm': True, 'two_rdm': True}),
           'bp_obs_hirsch.npz', 16)


def make_direct():
    """ekt.py on random G pairs: real vectors (M = 24, nL = 30) and complex ones (M = 20, nL = 24)."""
    out = {}
    rng = numpy.random.RandomState(99)
    for tag, M, nL, cplx in (('R_', 24, 30, False), ('C_', 20, 24, True)):
        L = rng.normal(size=(nL, M, M)) * (0.4 / numpy.sqrt(M))
        if cplx:
            L = L + 1j * rng.normal(size=(nL, M, M)) * (0.4 / numpy.sqrt(M))
        h = rng.normal(size=(M, M))
        h1 = 0.5 * (h + h.T)
        for i in range(2):
            Ga = rng.normal(size=(M, M)) + 1j * rng.normal(size=(M, M))
            Gb = rng.normal(size=(M, M)) + 1j * rng.normal(size=(M, M))
            out[tag + 'Ga%d' % i] = Ga
            out[tag + 'Gb%d' % i] = Gb
            out[tag + 'F1p%d' % i] = ekt_1p_fock_opt(h1, L, Ga, Gb)
            out[tag + 'F1h%d' % i] = ekt_1h_fock_opt(h1, L, Ga, Gb)
        out[tag + 'L'] = L
        out[tag + 'h1'] = h1
    mg.save('bp_obs_direct.npz', out)


FIXTURES = [
    ('bp_obs_generic.npz', lambda: traj_generic('bp_obs_generic.npz', {'one_rdm': True, 'two_rdm': True,
                                                                        'evaluate_ekt': True})),
    ('bp_obs_split.npz', lambda: traj_generic('bp_obs_split.npz', {'one_rdm': True, 'two_rdm': True,
                                                                    'evaluate_ekt': True, 'nsplit': 2}, tau_bp=0.03)),
    ('bp_obs_quirk.npz', lambda: traj_generic('bp_obs_quirk.npz', {'one_rdm': False, 'evaluate_ekt': True})),
    ('bp_obs_ueg.npz', make_ueg),
    ('bp_obs_hirsch.npz', make_hirsch),
    ('bp_obs_direct.npz', make_direct),
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
        if os.path.exists(os.path.join(mg.OUT, 'scratch.npz')):
            os.remove(os.path.join(mg.OUT, 'scratch.npz'))
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
