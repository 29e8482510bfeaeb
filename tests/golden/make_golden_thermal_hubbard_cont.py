#!/usr/bin/env python3
"""Golden fixture for the finite-temperature path of the Hubbard model with continuous fields, from the genuine
reference (qmc/thermal_afqmc.py, thermal_propagation/continuous.py, thermal_propagation/hubbard.py HubbardContinuous,
walkers/thermal.py, walkers/stack.py, trial_density_matrices/onebody.py): full-rank walkers, phaseless, force bias on,
`one_body` trial (dense), the charge form.

  thermal_hubbard_cont.npz
    a<k>_*  one ThermalWalker driven slice by slice by Continuous.propagate_walker, 10 slices:
              k  lattice  M   nup = ndown  U   mu   dt    stack_size  bins
              0  2 x 2    4   2            4   1    0.05  10          1
              1  2 x 2    4   2            4   1    0.05  1           10
              2  3 x 3    9   4            4   1    0.05  5           2
              3  3 x 3    9   4            4   1    0.05  1           10
              4  4 x 4    16  7            4   1    0.05  2           5
              5  4 x 4    16  7            4   1    0.05  10          1
              6  6 x 6    36  15           4   1    0.05  5           2      scalars only (no per-slice G)
              7  3 x 3    9   4            see A_CASES: a time step and a U at which the clip fires and a walker is killed
            per slice xi, xbar (clipped), cmf, cfb, M0, the weight, and where M <= 16 G and the stack's `left` of the
            slice's bin (real); once: the trial's mu, dmat,
            dmat_inv, BH1, mf_shift, mf_const_fac, the trial walker's G and M0, the final (E, T, V) and nav, the
            number of clipped components and of kills.
    b<k>_*  ThermalAFQMC over two paths with propagator: {hubbard_stratonovich: 'continuous'}, U = 4, mu = 1,
            dt = 0.05, beta = 1, pop_control_freq 5, seed b<k>_seed:
              k  lattice  nup = ndown  stack_size  walkers
              0  3 x 3    4            5           8
              1  4 x 4    7            5           6
            the estimator rows (Time zeroed), the weights of every walker after every propagate_walker call (before
            the cap), for every comb event the uniform, the weights it saw and parent_ix, and the propagator's count of
            clipped components.  The fields are not stored: numpy.random seeded with b<k>_seed reproduces them
            (checked here by replaying the stream).
    margins  no comb tooth within 1e-6 (relative to the total weight) of a cumulative weight, no cosine factor within
            1e-6 of 0 unless below -1e-3, no |xbar_i| within 1e-6 of the clip's bound 1 before the clip: asserted here
            for every case, so that a rounding difference cannot change a parent, a kill or the clip count.  Every case
            is also asserted to have run to the end with finite rows.

Uses the import recipe of make_golden.py (which it imports and does not change); runs only where the reference is
available.

Usage:  python tests/golden/make_golden_thermal_hubbard_cont.py            (writes tests/golden/thermal_hubbard_cont.npz)
        python tests/golden/make_golden_thermal_hubbard_cont.py --check    regenerate into a scratch directory and compare
"""
import math
import os
import shutil
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg                                                 # noqa: E402  (prepares the reference)
from make_golden import Hubbard, dotdict, h5py                           # noqa: E402
import pauxy.thermal_propagation.continuous as contmod                   # noqa: E402
from pauxy.trial_density_matrices.onebody import OneBody                 # noqa: E402
from pauxy.thermal_propagation.continuous import Continuous              # noqa: E402
from pauxy.walkers.thermal import ThermalWalker                          # noqa: E402
from pauxy.estimators.thermal import one_rdm_from_G, particle_number     # noqa: E402
from pauxy.qmc.thermal_afqmc import ThermalAFQMC                         # noqa: E402

COS = []
XBAR_MARGIN = [numpy.inf]
NAME = 'thermal_hubbard_cont.npz'


class _Math(object):
    """The math module as continuous.py sees it, with every cosine factor recorded."""

    def __getattr__(self, name):
        return getattr(math, name)

    @staticmethod
    def cos(x):
        c = math.cos(x)
        COS.append(c)
        return c


contmod.math = _Math()

A_CASES = [  # nx, ny, nelec per spin, U, mu, dt, stack_size, seed
    (2, 2, 2, 4.0, 1.0, 0.05, 10, 7), (2, 2, 2, 4.0, 1.0, 0.05, 1, 8), (3, 3, 4, 4.0, 1.0, 0.05, 5, 9),
    (3, 3, 4, 4.0, 1.0, 0.05, 1, 10), (4, 4, 7, 4.0, 1.0, 0.05, 2, 11), (4, 4, 7, 4.0, 1.0, 0.05, 10, 12),
    (6, 6, 15, 4.0, 1.0, 0.05, 5, 13), (3, 3, 4, 12.0, 1.0, 0.25, 5, 14)]
B_CASES = [  # nx, ny, nelec per spin, stack_size, walkers, seed
    (3, 3, 4, 5, 8, 7), (4, 4, 7, 5, 6, 7)]
STORE_G_UP_TO = 16
NSLICE = 10


def check_cosines(tag):
    for c in COS:
        assert abs(c) > 1e-6 or c < -1e-3, (tag, c)
    kills = sum(1 for c in COS if c <= 0)
    del COS[:]
    return kills


def watch_force_bias(prop, seen):
    """Records the force bias (the clip rescales the array in place afterwards) and its distance from the bound."""
    bias = prop.propagator.construct_force_bias

    def rec_bias(system, P, trial):
        seen['xbar'] = bias(system, P, trial)
        XBAR_MARGIN[0] = min(XBAR_MARGIN[0], float(numpy.min(numpy.abs(numpy.abs(seen['xbar']) - 1.0))))
        seen['nclip'] = seen.get('nclip', 0) + int(numpy.sum(numpy.abs(seen['xbar']) > 1.0))
        return seen['xbar']
    prop.propagator.construct_force_bias = rec_bias


def case_a(out, k, nx, ny, ne, U, mu, dt, stack_size, seed):
    system = Hubbard({'nx': nx, 'ny': ny, 'U': U, 'mu': mu, 'nup': ne, 'ndown': ne}, verbose=False)
    beta = NSLICE * dt
    trial = OneBody(system, beta, dt, verbose=False)
    qmc = dotdict({'dt': dt, 'nstblz': 10})
    prop = Continuous({}, qmc, system, trial, verbose=False, lowrank=False)
    numpy.random.seed(seed)
    walker = ThermalWalker(system, trial, walker_opts={'stack_size': stack_size, 'low_rank': False}, verbose=False)
    assert walker.stack_size == stack_size and walker.num_slices == NSLICE
    assert not walker.stack.diagonal_trial
    M = system.nbasis
    pre = 'a%d_' % k
    assert numpy.max(numpy.abs(numpy.asarray(prop.BH1).imag)) == 0.0
    assert numpy.max(numpy.abs(numpy.asarray(trial.dmat).imag)) == 0.0
    out.update({pre + 'nx': nx, pre + 'ny': ny, pre + 'nelec': ne, pre + 'U': U, pre + 'mu_system': float(system.mu),
                pre + 'stack_size': stack_size, pre + 'beta': beta, pre + 'dt': dt, pre + 'mu': float(trial.mu),
                pre + 'seed': seed, pre + 'dmat': numpy.array(trial.dmat.real), pre + 'dmat_inv': numpy.array(trial.dmat_inv.real),
                pre + 'BH1': numpy.array(numpy.asarray(prop.BH1).real), pre + 'mf_shift': numpy.array(prop.propagator.mf_shift),
                pre + 'mf_core': complex(prop.propagator.mf_core), pre + 'mf_const_fac': complex(prop.mf_const_fac),
                pre + 'G0': walker.G.copy(), pre + 'M00': numpy.array(walker.M0)})
    seen = {}
    watch_force_bias(prop, seen)
    normal = numpy.random.normal

    def rec_normal(*a):
        seen['xi'] = normal(*a)
        return seen['xi']
    two_body = prop.two_body_propagator

    def rec_two_body(w, s, t):
        r = two_body(w, s, t)
        seen['cmf'], seen['cfb'] = r[0], r[1]
        return r
    numpy.random.normal, prop.two_body_propagator = rec_normal, rec_two_body
    names = ('xi', 'xbar', 'cmf', 'cfb', 'M0', 'weight') + (('G', 'left') if M <= STORE_G_UP_TO else ())
    assert numpy.max(numpy.abs(numpy.asarray(walker.stack.left).imag)) == 0.0
    rows = {n: [] for n in names}
    try:
        for ts in range(NSLICE):
            block = walker.stack.block
            prop.propagate_walker(system, walker, trial, 0)
            if 'left' in rows:
                rows['left'].append(numpy.array(walker.stack.left[block].real))
            for n in ('xi', 'xbar', 'cmf', 'cfb'):
                rows[n].append(numpy.array(seen[n]))
            if 'G' in rows:
                rows['G'].append(walker.G.copy())
            rows['M0'].append(numpy.array(walker.M0))
            rows['weight'].append(float(numpy.real(walker.weight)))
    finally:
        numpy.random.normal = normal
    assert walker.stack.time_slice == NSLICE                       # ran to the end
    assert numpy.all(numpy.isfinite(rows['weight']))
    assert seen.get('nclip', 0) == prop.nfb_trig
    kills = check_cosines(pre)
    E = numpy.array(walker.local_energy(system))
    nav = complex(particle_number(one_rdm_from_G(walker.G)))
    assert numpy.all(numpy.isfinite(E)) and numpy.isfinite(nav)
    out.update({pre + n: numpy.array(v) for n, v in rows.items()})
    out.update({pre + 'G_last': walker.G.copy(), pre + 'energy': E, pre + 'nav': nav, pre + 'nclip': int(prop.nfb_trig),
                pre + 'kills': kills})


def case_b(out, k, nx, ny, ne, stack_size, nwalkers, seed):
    options = {'verbosity': 0, 'get_sha1': False,
               'qmc': {'timestep': 0.05, 'beta': 1.0, 'num_walkers': nwalkers, 'blocks': 2, 'pop_control_freq': 5,
                       'rng_seed': seed},
               'model': {'name': 'Hubbard', 'nx': nx, 'ny': ny, 'U': 4.0, 'mu': 1.0, 'nup': ne, 'ndown': ne},
               'trial': {'name': 'one_body'},
               'walkers': {'stack_size': stack_size, 'low_rank': False},
               'propagator': {'hubbard_stratonovich': 'continuous'},
               'estimates': {'mixed': {}}}
    comm = type(mg.MPI.COMM_WORLD)()
    h5py._STORE.clear()
    afqmc = ThermalAFQMC(comm, options=options)
    assert isinstance(afqmc.propagators, Continuous)
    walk = afqmc.walk
    nslice = afqmc.qmc.ntime_slices
    weights, combs = [], []
    watch_force_bias(afqmc.propagators, {})
    inner = afqmc.propagators.propagate_walker

    def propagate_walker(system, w, ts, eshift):
        inner(system, w, ts, eshift)
        weights.append(float(numpy.real(w.weight)))
    afqmc.propagators.propagate_walker = propagate_walker
    comb = walk.comb
    random = numpy.random.random

    def rec_comb(c, wts):
        seen = []

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
        r, total = seen[0], sum(before)
        cprobs = numpy.cumsum(before)
        teeth = numpy.array([(i + r) * (total / walk.target_weight) for i in range(walk.target_weight)])
        assert numpy.min(numpy.abs(teeth[:, None] - cprobs[None, :-1])) > 1e-6 * total, 'a comb tooth on a boundary'
        parent = numpy.zeros(len(before), dtype=numpy.int32)
        for t in teeth:
            parent[numpy.searchsorted(cprobs, t, side='right')] += 1
        combs.append((r, before, parent))
    walk.comb = rec_comb
    afqmc.run(comm=comm, verbose=0)
    store = h5py._STORE[afqmc.estimators.filename]
    keys = sorted(kk for kk in store if kk.startswith('basic/energies/'))
    blocks = numpy.array([store[kk] for kk in keys])
    assert blocks.shape == (3, 12), blocks.shape                  # ran to the end: the start and both paths
    assert numpy.all(numpy.isfinite(blocks))
    assert len(weights) == 2 * nslice * nwalkers and len(combs) >= 2
    blocks[:, -1] = 0
    kills = check_cosines('b%d' % k)
    # the stream: nfields normals per walker and slice in walker order, one uniform per comb event
    rs = numpy.random.RandomState(seed)
    ic = 0
    for _ in range(2):
        for ts in range(nslice):
            rs.normal(0.0, 1.0, (nwalkers, afqmc.system.nfields))
            if ts % afqmc.qmc.npop_control == 0 and ts != 0:
                assert rs.random_sample() == combs[ic][0]
                ic += 1
    assert ic == len(combs)
    pre = 'b%d_' % k
    out.update({pre + 'nx': nx, pre + 'ny': ny, pre + 'nelec': ne, pre + 'U': 4.0, pre + 'beta': 1.0, pre + 'mu_system': 1.0,
                pre + 'dt': 0.05, pre + 'stack_size': int(walk.walkers[0].stack_size), pre + 'nwalkers': nwalkers,
                pre + 'seed': seed, pre + 'npop_control': int(afqmc.qmc.npop_control), pre + 'ntime_slices': int(nslice),
                pre + 'mu': float(afqmc.trial.mu), pre + 'blocks': blocks,
                pre + 'header': numpy.array(afqmc.estimators.estimators['mixed'].header),
                pre + 'weights': numpy.array(weights).reshape(2 * nslice, nwalkers),
                pre + 'comb_r': numpy.array([c[0] for c in combs]),
                pre + 'comb_weights': numpy.array([c[1] for c in combs]),
                pre + 'parent_ix': numpy.array([c[2] for c in combs]), pre + 'kills': kills,
                pre + 'nclip': int(afqmc.propagators.nfb_trig)})


def make_thermal_hubbard_cont():
    out = {}
    XBAR_MARGIN[0] = numpy.inf
    for k, case in enumerate(A_CASES):
        case_a(out, k, *case)
    for k, case in enumerate(B_CASES):
        case_b(out, k, *case)
    assert out['a7_nclip'] > 0, 'the clip case does not clip'
    assert out['a7_kills'] > 0, 'the kill case kills no walker'
    assert XBAR_MARGIN[0] > 1e-6, XBAR_MARGIN[0]
    out['xbar_margin'] = float(XBAR_MARGIN[0])
    mg.save(NAME, out)
    assert os.path.getsize(os.path.join(mg.OUT, NAME)) < 1000 * 1000


FIXTURES = [(NAME, make_thermal_hubbard_cont)]


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
