#!/usr/bin/env python3
"""Golden fixtures for back-propagated UEG / Hubbard energies and the UEG structure factor, from the genuine reference.

Uses the import recipe and the recorders of make_golden.py (which it imports and does not change); runs only where
the reference is available.  Tests read the .npz files this writes.

  ueg_sf_traj.npz        traj_bp_ueg's run (M = 33, nq = 256, 10 walkers, tau_bp = 4 steps) with evaluate_energy and
                         two_rdm: 'structure_factor': energies_<n> and two_rdm_<n> of every window.  New outputs only;
                         the run itself is bitwise traj_bp_ueg.npz's (checked here)
  hubbard_bp_energy.npz  traj_hirsch_bp's run (discrete fields, 4x4, tau_bp = 4 steps) with evaluate_energy:
                         energies_<n> of every window; the run itself is bitwise traj_hirsch_bp.npz's (checked here)
  ueg_sf_direct.npz      local_energy_ueg(system, G, two_rdm=...) on the back-propagated Green's functions of
                         bp_obs_ueg.npz (bp_win0_G) and on random dense complex G, with the default (first nup plane
                         waves) and the thermal: True (all plane waves) index lists, for an unpolarised and a polarised
                         gas and a second cutoff; the thermal lists themselves are stored

The reference's BackPropagation.update_uhf calls local_energy(system, G, opt=False, two_rdm=...), and the dispatcher
has no `opt` keyword (TypeError): the reference cannot produce these outputs as it stands.  For these runs the name
`local_energy` of the reference's back_propagation module is wrapped at run time to drop that keyword; everything
else is the reference's own code.

Usage:  python tests/golden/make_golden_ueg_sf.py            (writes the three fixtures)
        python tests/golden/make_golden_ueg_sf.py --check    regenerate into a scratch directory and compare
"""
import os
import shutil
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg                                                 # noqa: E402  (prepares the reference)
from make_golden import AFQMC, UEG                                       # noqa: E402
import pauxy.estimators.back_propagation as ref_bp                       # noqa: E402
from pauxy.estimators.ueg import local_energy_ueg                        # noqa: E402

_local_energy = ref_bp.local_energy


def _local_energy_no_opt(system, G, opt=None, **kw):
    return _local_energy(system, G, **kw)


ref_bp.local_energy = _local_energy_no_opt


def _with_bp_options(extra):
    """An AFQMC constructor that adds ``extra`` to the back_propagated options of the input it is handed."""
    def make(*a, **k):
        opts = k.get('options')
        for sec in ('estimates', 'estimator', 'estimators'):
            if opts is not None and 'back_propagated' in opts.get(sec, {}):
                opts[sec]['back_propagated'].update(extra)
        return AFQMC(*a, **k)
    return make


def _series(store, kind, sp):
    keys = sorted((k for k in store if k.startswith('back_propagated/%s_%d/' % (kind, sp))),
                  key=lambda k: int(k.rsplit('/', 1)[1]))
    return numpy.array([store[k] for k in keys])


def _rerun(make, extra, name, base, kinds):
    """One of make_golden's BP runs with ``extra`` added to its back_propagated options: checks that everything the
    committed fixture ``base`` of that run holds came out bitwise the same and stores the series ``kinds``."""
    saved = {}
    real_save, real_afqmc = mg.save, mg.AFQMC
    mg.save = lambda nm, out: saved.update(out)
    mg.AFQMC = _with_bp_options(extra)
    mg.h5py._STORE.clear()
    try:
        make()
    finally:
        mg.save, mg.AFQMC = real_save, real_afqmc
    stores = [s for s in mg.h5py._STORE.values() if any(k.startswith('back_propagated/') for k in s)]
    assert len(stores) == 1
    b = numpy.load(os.path.join(mg.HERE, base), allow_pickle=False)
    saved['blocks'] = numpy.array(saved['blocks'])
    saved['blocks'][:, -1] = 0                      # the wall clock, zeroed by save() as well
    saved['final_estimates'] = numpy.array(saved['final_estimates'])
    saved['final_estimates'][9] = 0
    for k in b.files:
        assert numpy.array_equal(b[k], saved[k], equal_nan=b[k].dtype.kind in 'fc'), k
    nbp = int(saved['nbp'])
    out = {'nbp': nbp}
    den = _series(stores[0], 'denominator', nbp)
    assert len(den) > 0 and numpy.array_equal(den.reshape(len(den)), b['bp_denominator'])
    for kind in kinds:
        s = _series(stores[0], kind, nbp)
        assert len(s) == len(den), kind
        out['bp_' + kind] = s
    mg.save(name, out)


def make_traj():
    # (the literal below is the very object the reference's `is not "structure_factor"` compares with)
    _rerun(lambda: mg.make_traj_bp_ueg('scratch.npz'), {'evaluate_energy': True, 'two_rdm': 'structure_factor'},
           'ueg_sf_traj.npz', 'traj_bp_ueg.npz', ('energies', 'two_rdm'))


def make_hubbard():
    _rerun(lambda: mg.make_traj_hirsch('scratch.npz', blocks=4, bp={'tau_bp': 0.04, 'one_rdm': True}),
           {'evaluate_energy': True}, 'hubbard_bp_energy.npz', 'traj_hirsch_bp.npz', ('energies',))


def _lists(system, out, tag):
    for nm in ('ikpq_i', 'ikpq_kpq', 'ipmq_i', 'ipmq_pmq'):
        ls = getattr(system, nm)
        out[tag + nm + '_off'] = numpy.concatenate([[0], numpy.cumsum([len(x) for x in ls])]).astype(numpy.int64)
        out[tag + nm] = (numpy.concatenate([numpy.asarray(x, dtype=numpy.int64) for x in ls])
                         if sum(len(x) for x in ls) else numpy.zeros(0, dtype=numpy.int64))


def make_direct():
    out = {}
    rng = numpy.random.RandomState(2024)
    bp = numpy.load(os.path.join(mg.HERE, 'bp_obs_ueg.npz'), allow_pickle=False)
    cases = (('u', 2.44, 7, 7, 2.0), ('p', 2.44, 7, 3, 2.0), ('c', 2.0, 7, 7, 1.0))
    for tag, rs, nup, ndown, ecut in cases:
        for kind, thermal in (('t', False), ('f', True)):
            system = UEG({'rs': rs, 'nup': nup, 'ndown': ndown, 'ecut': ecut, 'thermal': thermal}, verbose=False)
            M, nq = system.nbasis, len(system.qvecs)
            key = tag + kind + '_'
            if kind == 't':
                out[tag + '_sys'] = numpy.array([rs, nup, ndown, ecut])
                G = [rng.normal(size=(2, M, M)) + 1j * rng.normal(size=(2, M, M)) for _ in range(2)]
                if tag == 'u':
                    assert bp['bp_win0_G'].shape[1:] == (2, M, M)
                    G = [bp['bp_win0_G'][0], bp['bp_win0_G'][3]] + G
                out[tag + '_G'] = numpy.array(G)
            else:
                _lists(system, out, key)
            E, two = [], []
            for g in out[tag + '_G']:
                t = numpy.zeros((2, 2, nq), dtype=numpy.complex128)
                E.append(numpy.array(local_energy_ueg(system, g, two_rdm=t)))
                two.append(t)
            out[key + 'E'] = numpy.array(E)
            out[key + 'two_rdm'] = numpy.array(two)
    mg.save('ueg_sf_direct.npz', out)


FIXTURES = [
    ('ueg_sf_traj.npz', make_traj),
    ('hubbard_bp_energy.npz', make_hubbard),
    ('ueg_sf_direct.npz', make_direct),
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
