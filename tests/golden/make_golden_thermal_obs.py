#!/usr/bin/env python3
"""Golden fixture for the mixed estimator's thermal observables, from the genuine reference (estimators/mixed.py:180-233,
279-288 with walkers/thermal.py:472-547 and qmc/thermal_afqmc.py): `one_rdm: True`, `two_rdm: 'structure_factor'` (UEG)
and `average_gf: True`, through ThermalAFQMC over two paths with 6 walkers, seed 8, dt = 0.05, pop_control_freq 5.

  thermal_obs.npz, one group of keys per case <c>_*:
      c     system                                          beta  stack_size (bins)  mixed options
      ua    UEG ecut 1.0 (M = 19), 2 + 2, rs 1, mu 0.245    1.0   4  (5)             one_rdm, structure_factor
      ub    as ua                                           1.0   4  (5)             one_rdm, structure_factor, average_gf
      uc    UEG ecut 0.5 (M = 7), 1 + 1, rs 1, mu 0.245     0.5   1  (10)            one_rdm, structure_factor, average_gf
      ud    as uc                                           0.5   10 (1)             one_rdm, structure_factor, average_gf
      ha    Hubbard 3x3, 4 + 4, U = 4, mu 1.0, discrete     1.0   5  (4)             one_rdm
      hb    as ha                                           1.0   5  (4)             one_rdm, average_gf
      hc    as ha, hubbard_stratonovich: 'continuous'       1.0   5  (4)             one_rdm, average_gf
    blocks      the estimator rows [3, 12] (Time zeroed).  With average_gf the reference never adds to EDenom
                (mixed.py:182-199 has no such line): EDenom is 0 and ETotal, E1Body, E2Body are +-inf or NaN there.
    estimates   the raw `estimates` vector after every Mixed.update, before print_step divides [3, nreg + RDM sizes]
                (the time slot zeroed)
    one_rdm, two_rdm   the pushed blocks basic/one_rdm/<n> [3, 2, M, M], basic/two_rdm/<n> [3, 2, 2, nq]
    weights     every walker's weight at every update [3, nw]
    per_bin     every walker's (E, T, V, nav) of every Green's function the update evaluates [3, bins, nw, 4], complex
                as the walkers' are (the estimator keeps the real parts): the stack_length of the sweep with average_gf,
                else one (the walker's current slice)
    sums        their sums over the bins in ts order [3, nw, 4]
    stacks      the first two walkers' bins at the end of path 1 [2, bins, 2, M, M], for the kernel-level tests
    and what the run was made from (mu of the trial, the header, the options' numbers).
  margins  no comb tooth within 1e-6 (relative to the total weight) of a cumulative weight; no cosine factor within 1e-6
           of 0 unless below -1e-3; the discrete fields' uniforms no nearer than 1e-6 to their thresholds; the
           continuous Hubbard force bias no nearer than 1e-6 to its clip: asserted for every case, so that a rounding
           difference cannot change a parent, a kill or a field.  Every case is also asserted to have run to the end.

Uses the import recipe of make_golden.py and the watchers of the three thermal generators (which it imports and does
not change); runs only where the reference is available.

Usage:  python tests/golden/make_golden_thermal_obs.py            (writes tests/golden/thermal_obs.npz)
        python tests/golden/make_golden_thermal_obs.py --check    regenerate into a scratch directory and compare
"""
import os
import shutil
import sys
import warnings

import numpy

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg                                                 # noqa: E402  (prepares the reference)
from make_golden import h5py                                             # noqa: E402
import make_golden_thermal as gt                                         # noqa: E402  (uniform margins)
import make_golden_thermal_ueg as gu                                     # noqa: E402  (planewave.py's cosines)
import make_golden_thermal_hubbard_cont as gc                            # noqa: E402  (continuous.py's cosines, the clip)
from pauxy.estimators.thermal import one_rdm_from_G, particle_number     # noqa: E402
from pauxy.qmc.thermal_afqmc import ThermalAFQMC                         # noqa: E402

NAME = 'thermal_obs.npz'
NWALKERS, SEED, DT = 6, 8, 0.05
UEG19 = {'name': 'UEG', 'rs': 1.0, 'ecut': 1.0, 'nup': 2, 'ndown': 2, 'mu': 0.245}
UEG7 = {'name': 'UEG', 'rs': 1.0, 'ecut': 0.5, 'nup': 1, 'ndown': 1, 'mu': 0.245}
HUB = {'name': 'Hubbard', 'nx': 3, 'ny': 3, 'U': 4.0, 'mu': 1.0, 'nup': 4, 'ndown': 4}
SF = {'one_rdm': True, 'two_rdm': 'structure_factor'}
CASES = [  # tag, model, beta, stack_size, propagator options, mixed options
    ('ua', UEG19, 1.0, 4, {'optimised': True}, dict(SF)),
    ('ub', UEG19, 1.0, 4, {'optimised': True}, dict(SF, average_gf=True)),
    ('uc', UEG7, 0.5, 1, {'optimised': True}, dict(SF, average_gf=True)),
    ('ud', UEG7, 0.5, 10, {'optimised': True}, dict(SF, average_gf=True)),
    ('ha', HUB, 1.0, 5, {}, {'one_rdm': True}),
    ('hb', HUB, 1.0, 5, {}, {'one_rdm': True, 'average_gf': True}),
    ('hc', HUB, 1.0, 5, {'hubbard_stratonovich': 'continuous'}, {'one_rdm': True, 'average_gf': True}),
]


def watch_comb(walk, combs):
    """Every comb event: the uniform, the weights it saw, and no tooth on a boundary."""
    comb = walk.comb

    def rec_comb(c, wts):
        seen, random = [], numpy.random.random

        def rec_random(*a):
            seen.append(random(*a))
            return seen[-1]
        numpy.random.random = rec_random
        try:
            before = numpy.array(wts)
            comb(c, wts)
        finally:
            numpy.random.random = random
        assert len(seen) == 1
        r, total = float(seen[0]), sum(before)
        cprobs = numpy.cumsum(before)
        teeth = numpy.array([(i + r) * (total / walk.target_weight) for i in range(walk.target_weight)])
        assert numpy.min(numpy.abs(teeth[:, None] - cprobs[None, :-1])) > 1e-6 * total, 'a comb tooth on a boundary'
        combs.append(r)
    walk.comb = rec_comb


def measure(system, trial, walk, average_gf):
    """What Mixed.update is about to evaluate, walker by walker, by the walkers' own methods: the Green's functions are
    functions of the stacks alone, so the update that follows finds and leaves what it would have."""
    per_bin = []
    for w in walk.walkers:
        rows = []
        for ts in (range(w.stack_length) if average_gf else [None]):
            w.greens_function(trial, slice_ix=None if ts is None else ts * w.stack_size)
            E, T, V = w.local_energy(system)
            nav = particle_number(one_rdm_from_G(w.G))
            rows.append([E, T, V, nav])
        per_bin.append(rows)
    per_bin = numpy.array(per_bin, dtype=complex).transpose(1, 0, 2)     # [bins, nw, 4]
    sums = numpy.zeros(per_bin.shape[1:], dtype=complex)
    for b in per_bin:
        sums += b
    return per_bin, sums


def case(out, tag, model, beta, stack_size, prop_opts, mixed_opts):
    options = {'verbosity': 0, 'get_sha1': False,
               'qmc': {'timestep': DT, 'beta': beta, 'num_walkers': NWALKERS, 'blocks': 2, 'pop_control_freq': 5,
                       'rng_seed': SEED},
               'model': dict(model), 'trial': {'name': 'one_body'},
               'walkers': {'stack_size': stack_size, 'low_rank': False},
               'propagator': dict(prop_opts), 'estimates': {'mixed': dict(mixed_opts)}}
    average_gf = bool(mixed_opts.get('average_gf', False))
    comm = type(mg.MPI.COMM_WORLD)()
    h5py._STORE.clear()
    afqmc = ThermalAFQMC(comm, options=options)
    walk, mixed = afqmc.walk, afqmc.estimators.estimators['mixed']
    nbins = afqmc.qmc.ntime_slices // stack_size
    assert int(walk.walkers[0].stack_size) == stack_size and int(walk.walkers[0].stack_length) == nbins
    assert bool(mixed.average_gf) == average_gf
    combs, rec = [], {'estimates': [], 'weights': [], 'per_bin': [], 'sums': [], 'stacks': None}
    watch_comb(walk, combs)
    discrete = model['name'] == 'Hubbard' and 'hubbard_stratonovich' not in prop_opts
    if model['name'] == 'Hubbard' and not discrete:
        gc.watch_force_bias(afqmc.propagators, {})
    update = mixed.update

    def rec_update(system, qmc, trial, psi, step, free_projection=False):
        rec['weights'].append([float(numpy.real(w.weight)) for w in psi.walkers])
        per_bin, sums = measure(system, trial, psi, average_gf)
        rec['per_bin'].append(per_bin)
        rec['sums'].append(sums)
        if step == 1:
            assert all(int(w.stack.time_slice) == afqmc.qmc.ntime_slices for w in psi.walkers[:2])
            rec['stacks'] = numpy.array([numpy.array(w.stack.stack) for w in psi.walkers[:2]])
        update(system, qmc, trial, psi, step, free_projection)
        es = numpy.array(mixed.estimates)
        es[mixed.names.time] = 0
        rec['estimates'].append(es)
    mixed.update = rec_update
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                                  # (average_gf: the reference divides by EDenom = 0)
        with numpy.errstate(all='ignore'):
            if discrete:
                gt.MARGIN[0] = numpy.inf
                with gt.Stream() as st:
                    gt.watch_margins(afqmc.propagators, lambda: st)
                    afqmc.run(comm=comm, verbose=0)
                assert gt.MARGIN[0] > 1e-6, (tag, gt.MARGIN[0])
            else:
                afqmc.run(comm=comm, verbose=0)
    gu.check_cosines(tag)
    gc.check_cosines(tag)
    store = h5py._STORE[afqmc.estimators.filename]

    def pushed(group):
        keys = sorted((k for k in store if k.startswith('basic/%s/' % group)), key=lambda k: int(k.rsplit('/', 1)[1]))
        return numpy.array([store[k] for k in keys])
    blocks = pushed('energies')
    assert blocks.shape == (3, 12), blocks.shape                         # ran to the end: the start and both paths
    blocks[:, -1] = 0
    assert len(rec['estimates']) == 3 and len(combs) >= 2 and rec['stacks'] is not None
    ns = mixed.names
    finite = [ns.uweight, ns.weight, ns.enumer, ns.e1b, ns.e2b, ns.nav]
    assert numpy.all(numpy.isfinite(numpy.array(rec['estimates'])[:, finite]))
    one = pushed('one_rdm')
    M = afqmc.system.nbasis
    assert one.shape == (3, 2, M, M) and numpy.all(numpy.isfinite(one))
    pre = tag + '_'
    out.update({pre + 'blocks': blocks, pre + 'estimates': numpy.array(rec['estimates']), pre + 'one_rdm': one,
                pre + 'weights': numpy.array(rec['weights']), pre + 'per_bin': numpy.array(rec['per_bin']),
                pre + 'sums': numpy.array(rec['sums']), pre + 'stacks': rec['stacks'],
                pre + 'header': numpy.array(mixed.header), pre + 'mu': float(afqmc.trial.mu), pre + 'beta': beta,
                pre + 'dt': DT, pre + 'stack_size': stack_size, pre + 'nbins': nbins, pre + 'nwalkers': NWALKERS,
                pre + 'seed': SEED, pre + 'npop_control': int(afqmc.qmc.npop_control),
                pre + 'ntime_slices': int(afqmc.qmc.ntime_slices), pre + 'average_gf': average_gf,
                pre + 'ncombs': len(combs), pre + 'nreg': int(mixed.nreg)})
    if 'two_rdm' in mixed_opts:
        two = pushed('two_rdm')
        assert two.shape == (3, 2, 2, len(afqmc.system.qvecs)) and numpy.all(numpy.isfinite(two))
        out[pre + 'two_rdm'] = two
    if average_gf:
        assert numpy.all(numpy.array(rec['estimates'])[:, ns.edenom] == 0)   # the quirk the package does not follow


def make_thermal_obs():
    out = {}
    gc.XBAR_MARGIN[0] = numpy.inf
    for c in CASES:
        case(out, *c)
    assert gc.XBAR_MARGIN[0] > 1e-6, gc.XBAR_MARGIN[0]
    out['cases'] = numpy.array([c[0] for c in CASES])
    mg.save(NAME, out)
    assert os.path.getsize(os.path.join(mg.OUT, NAME)) < 1000 * 1000


FIXTURES = [(NAME, make_thermal_obs)]


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
            print('%-24s %s' % (name, 'identical to the committed fixture' if not bad else 'DIFFERS: ' + '; '.join(bad[:6])))
            failed += bool(bad)
        else:
            print('%-24s %d bytes' % (name, os.path.getsize(os.path.join(mg.OUT, name))))
    if check:
        shutil.rmtree(mg.OUT, ignore_errors=True)
        print('%d of %d fixtures differ' % (failed, len(FIXTURES)) if failed else 'all %d fixtures reproduce' % len(FIXTURES))
        sys.exit(1 if failed else 0)
