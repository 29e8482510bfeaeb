#!/usr/bin/env python3
"""Golden fixture for the finite-temperature Hubbard path with discrete fields beyond 64 sites, from the genuine
reference (thermal_propagation/hubbard.py, walkers/thermal.py, qmc/thermal_afqmc.py), for the delayed-update route
(walkers: {delayed_updates: True}, AFQ_THERMAL_DELAYED).

  thermal_hubbard_large.npz
    c_*   one ThermalWalker with ThermalDiscrete.propagate_walker on 5 x 13 (65 sites), U = 4, mu = 1, beta = 0.5,
          dt = 0.05, stack_size 5, nstblz 5: the uniforms, the fields and the weight of every slice, G after slices 1, 5
          and 10, the final (E, T, V) and nav.
    e_*   ThermalAFQMC on 5 x 13, 4 walkers, walkers: {stack_size: 5}, pop_control_freq 5, two paths: every draw in
          the order drawn with the positions of the comb's r, the estimator rows (the Time column zeroed).
  thermal_hubbard_large_d.npz
    d_*   case c on 10 x 10; G after slices 5 and 10 only.
  The trial's and the propagator's matrices are stored where tests/thermal_ref.hubbard_kinetic, one_body_dmat and
  hubbard_auxf do not rebuild the reference's to the bit from (nx, ny, U, dt, mu, the trial's mu): auxf is rebuilt, and on
  10 x 10 T and BH1; the others are stored for c and d (`*_rebuilt` records it, and REBUILT asserts which case holds).  Case e stores none: the driver builds its own.
  min_margin   the smallest |u - p_0 / norm| over every recorded decision of both files, asserted > 1e-6: the seed
          (SEED) is one for which the reference alone satisfies that.

Uses make_golden_thermal.py's recorders (which it imports and does not change); runs only where the reference is
available.

Usage:  python tests/golden/make_golden_thermal_delayed.py            (writes the two files)
        python tests/golden/make_golden_thermal_delayed.py --check    regenerate into a scratch directory and compare
"""
import os
import shutil
import sys

import numpy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_thermal as mt                                         # noqa: E402  (prepares the reference)
from make_golden_thermal import (Hubbard, OneBody, Stream, ThermalAFQMC, ThermalDiscrete, ThermalWalker,   # noqa: E402
                                 dotdict, fields_of, h5py, mg, one_rdm_from_G, particle_number, watch_margins)

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import thermal_ref as tr                                      # noqa: E402

SEED = 11                       # (seed 7, the 4 x 4 fixture's, leaves a decision of case e within 3.2e-7 of its threshold)
LATTICES = {'c': (5, 13, 30, (1, 5, 10)), 'd': (10, 10, 45, (5, 10)), 'e': (5, 13, 30, None)}
U, MU, BETA, DT, STACK, NSTBLZ = 4, 1.0, 0.5, 0.05, 5, 5
MARGIN = mt.MARGIN
# which of (T, dmat, dmat_inv, BH1, auxf) tests/thermal_ref rebuilds to the bit, per case
# (the reference numbers the sites of an nx != ny lattice in another order; its dmat is expm(-dt H1) exp(dt mu) and its
# dmat_inv scipy's inverse, where thermal_ref takes expm(-+dt (H1 - mu I)))
REBUILT = {'c': [False, False, False, False, True], 'd': [True, False, False, True, True],
           'e': [False, False, False, False, True]}


def model(tag):
    nx, ny, ne, _ = LATTICES[tag]
    return {'nx': nx, 'ny': ny, 'U': U, 'mu': MU, 'nup': ne, 'ndown': ne}


def rebuilt(out, system, trial, prop, tag, store=True):
    """Which of the reference's T, dmat, dmat_inv, BH1 and auxf tests/thermal_ref rebuilds to the bit from the case's
    scalars: `<tag>_rebuilt` [5] records it, and a matrix that is not rebuilt is stored (`<tag>_T`, `_dmat`, ...)."""
    nx, ny, _, _ = LATTICES[tag]
    T = tr.hubbard_kinetic(nx, ny)
    H1 = numpy.array([T, T])
    BT, BT_inv = tr.one_body_dmat(H1, float(trial.mu), DT)
    auxf = tr.hubbard_auxf(float(system.U), DT, float(system.mu), float(trial.mu))
    pairs = [('T', system.T.real, H1), ('dmat', trial.dmat.real, BT), ('dmat_inv', trial.dmat_inv.real, BT_inv),
             ('BH1', numpy.array(prop.BH1), BT), ('auxf', numpy.array(prop.auxf), auxf)]
    same = [bool(numpy.array_equal(ref, mine)) for _, ref, mine in pairs]
    assert same == REBUILT[tag], (tag, same)                  # which case holds is part of the recipe
    out[tag + '_rebuilt'] = numpy.array(same)
    out[tag + '_rebuilt_names'] = numpy.array([n for n, _, _ in pairs])
    if store:
        for (name, ref, _), ok in zip(pairs, same):
            if not ok:
                out[tag + '_' + name] = numpy.array(ref)


def one_walker(out, tag):
    nx, ny, ne, keep = LATTICES[tag]
    system = Hubbard(model(tag), verbose=False)
    nslice = int(round(BETA / DT))
    trial = OneBody(system, BETA, DT)
    prop = ThermalDiscrete(system, trial, dotdict({'dt': DT, 'nstblz': NSTBLZ}), verbose=False)
    assert not numpy.iscomplexobj(prop.auxf) and not numpy.iscomplexobj(prop.BH1)
    cur = {}
    watch_margins(prop, lambda: cur['st'])
    numpy.random.seed(SEED)
    walker = ThermalWalker(system, trial, walker_opts={'stack_size': STACK, 'low_rank': False}, verbose=False)
    assert walker.stack_size == STACK and numpy.max(numpy.abs(walker.G.imag)) == 0.0
    Gs, ws, us, xs = [], [], [], []
    for ts in range(nslice):
        with Stream() as st:
            cur['st'] = st
            prop.propagate_walker(system, walker, ts, 0)
        assert len(st.drawn) == system.nbasis
        us.append(st.drawn)
        xs.append(fields_of(prop.BV, prop.auxf))
        assert numpy.max(numpy.abs(walker.G.imag)) == 0.0
        if ts + 1 in keep:
            Gs.append(walker.G.real.copy())
        ws.append(float(numpy.real(walker.weight)))
    E = numpy.array(walker.local_energy(system)).real
    nav = float(particle_number(one_rdm_from_G(walker.G)).real)
    out.update({tag + '_nx': nx, tag + '_ny': ny, tag + '_U': float(system.U), tag + '_mu_system': float(system.mu),
                tag + '_nelec': numpy.array([ne, ne]), tag + '_beta': BETA, tag + '_dt': DT, tag + '_stack_size': STACK,
                tag + '_nstblz': NSTBLZ, tag + '_num_slices': nslice, tag + '_mu': float(trial.mu),
                tag + '_G_slices': numpy.array(keep),
                tag + '_G': numpy.array(Gs), tag + '_weight': numpy.array(ws), tag + '_u': numpy.array(us),
                tag + '_fields': numpy.array(xs), tag + '_energy': E, tag + '_nav': nav, tag + '_seed': SEED})
    rebuilt(out, system, trial, prop, tag)


def driver(out, tag='e'):
    options = {'verbosity': 0, 'get_sha1': False,
               'qmc': {'timestep': DT, 'beta': BETA, 'num_walkers': 4, 'blocks': 2, 'pop_control_freq': 5,
                       'rng_seed': SEED},
               'model': dict(model(tag), name='Hubbard'),
               'trial': {'name': 'one_body'},
               'walkers': {'stack_size': STACK},
               'estimates': {'mixed': {}}}
    comm = type(mg.MPI.COMM_WORLD)()
    h5py._STORE.clear()
    afqmc = ThermalAFQMC(comm, options=options)
    walk = afqmc.walk
    r_pos = []
    inner = walk.pop_control
    with Stream() as st:
        def pop_control(c):
            n = len(st.drawn)
            inner(c)
            if len(st.drawn) == n + 1:
                r_pos.append(n)
        walk.pop_control = pop_control
        watch_margins(afqmc.propagators, lambda: st)
        afqmc.run(comm=comm, verbose=0)
    store = h5py._STORE[afqmc.estimators.filename]
    keys = sorted(k for k in store if k.startswith('basic/energies/'))
    nx, ny, ne, _ = LATTICES[tag]
    out['e_blocks'] = numpy.array([store[k] for k in keys])
    out['e_header'] = numpy.array(afqmc.estimators.estimators['mixed'].header)
    out.update(e_draws=numpy.array(st.drawn), e_r_pos=numpy.array(r_pos, dtype=numpy.int64), e_nwalkers=4, e_beta=BETA,
               e_dt=DT, e_stack_size=int(walk.walkers[0].stack_size), e_nstblz=int(afqmc.qmc.nstblz),
               e_npop_control=int(afqmc.qmc.npop_control), e_paths=2, e_seed=SEED, e_mu=float(afqmc.trial.mu),
               e_nx=nx, e_ny=ny, e_U=float(afqmc.system.U), e_mu_system=float(afqmc.system.mu),
               e_nelec=numpy.array([ne, ne]), e_ntime_slices=int(afqmc.qmc.ntime_slices))
    rebuilt(out, afqmc.system, afqmc.trial, afqmc.propagators, tag, store=False)     # (the driver builds its own)
    assert len(out['e_blocks']) == 3 and out['e_blocks'].shape[1] == 12, out['e_blocks'].shape
    assert len(r_pos) >= 1


def finish(name, out):
    assert MARGIN[0] > 1e-6, MARGIN[0]
    out['min_margin'] = float(MARGIN[0])
    mg.save(name, out)
    assert os.path.getsize(os.path.join(mg.OUT, name)) < 1000 * 1000


def make_large():
    out = {}
    MARGIN[0] = numpy.inf
    one_walker(out, 'c')
    driver(out)
    finish('thermal_hubbard_large.npz', out)


def make_large_d():
    out = {}
    MARGIN[0] = numpy.inf
    one_walker(out, 'd')
    finish('thermal_hubbard_large_d.npz', out)


FIXTURES = [('thermal_hubbard_large.npz', make_large), ('thermal_hubbard_large_d.npz', make_large_d)]


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
            print('%-28s %s' % (name, 'identical to the committed fixture' if not bad else 'DIFFERS: ' + '; '.join(bad[:6])))
            failed += bool(bad)
        else:
            print('%-28s %d bytes' % (name, os.path.getsize(os.path.join(mg.OUT, name))))
    if check:
        shutil.rmtree(mg.OUT, ignore_errors=True)
        print('%d of %d fixtures differ' % (failed, len(FIXTURES)) if failed else 'all %d fixtures reproduce' % len(FIXTURES))
        sys.exit(1 if failed else 0)
