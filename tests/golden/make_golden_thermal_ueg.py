#!/usr/bin/env python3
"""Golden fixture for the finite-temperature path of the uniform electron gas with continuous fields, from the genuine
reference (qmc/thermal_afqmc.py, thermal_propagation/planewave.py, walkers/thermal.py, walkers/stack.py,
trial_density_matrices/onebody.py): full-rank walkers, phaseless, force bias on, `one_body` trial.

  thermal_ueg.npz
    a<k>_*  one ThermalWalker driven slice by slice by PlaneWave.propagate_walker, beta = 0.5, dt = 0.05 (10 slices):
              k  ecut  M   nup = ndown  rs   stack_size  bins
              0  0.5   7   1            1.0  10          1
              1  0.5   7   1            1.0  1           10
              2  1.0   19  2            1.0  5           2
              3  2.0   33  2            1.0  2           5
              4  1.0   19  7            4.0  5           2     fb_bound 0.01: the force-bias clip fires (a4_nclip > 0)
            per slice xi, xbar (clipped), cmf, cfb, G, M0 and the weight; the trial's mu, the diagonals of dmat, dmat_inv
            and BH1, mf_shift, the trial walker's G and M0, the final (E, T, V) and nav.
    b<k>_*  ThermalAFQMC over two paths, rs = 1, dt = 0.05, pop_control_freq 5, seed b<k>_seed:
              k  ecut  M   nup = ndown  beta  mu     stack_size  walkers
              0  1.0   19  2            1.0   0.245  4           12
              1  1.0   19  2            1.0   0.245  4           8       the cap fires for every walker on every slice
              2  2.0   33  2            1.0   0.245  5           12
              3  2.0   33  2            1.0   0.245  5           8
            the estimator rows (Time zeroed), the weights of every walker after every propagate_walker call (before
            the cap), and for every comb event the uniform, the weights it saw and parent_ix.  The fields are not
            stored: numpy.random seeded with b<k>_seed reproduces them (checked here by replaying the stream).
    margins  no comb tooth within 1e-6 (relative to the total weight) of a cumulative weight, no cosine factor within
            1e-6 of 0 unless below -1e-3: asserted here for every case, so that a rounding difference cannot change a
            parent or a kill.  Every case is also asserted to have run to the end.

Uses the import recipe of make_golden.py (which it imports and does not change); runs only where the reference is
available.

Usage:  python tests/golden/make_golden_thermal_ueg.py            (writes tests/golden/thermal_ueg.npz)
        python tests/golden/make_golden_thermal_ueg.py --check    regenerate into a scratch directory and compare
"""
import math
import os
import shutil
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg                                                 # noqa: E402  (prepares the reference)
from make_golden import UEG, dotdict, h5py                               # noqa: E402
import pauxy.thermal_propagation.planewave as pwmod                      # noqa: E402
from pauxy.trial_density_matrices.onebody import OneBody                 # noqa: E402
from pauxy.thermal_propagation.planewave import PlaneWave                # noqa: E402
from pauxy.walkers.thermal import ThermalWalker                          # noqa: E402
from pauxy.estimators.thermal import one_rdm_from_G, particle_number     # noqa: E402
from pauxy.qmc.thermal_afqmc import ThermalAFQMC                         # noqa: E402

COS = []


class _Math(object):
    """The math module as planewave.py sees it, with every cosine factor recorded."""

    def __getattr__(self, name):
        return getattr(math, name)

    @staticmethod
    def cos(x):
        c = math.cos(x)
        COS.append(c)
        return c


pwmod.math = _Math()

A_CASES = [  # ecut, nelec per spin, rs, stack_size, fb_bound (the force bias of these gases stays below 0.1)
    (0.5, 1, 1.0, 10, 1.0), (0.5, 1, 1.0, 1, 1.0), (1.0, 2, 1.0, 5, 1.0), (2.0, 2, 1.0, 2, 1.0), (1.0, 7, 4.0, 5, 0.01)]
B_CASES = [  # ecut, nelec per spin, beta, mu, stack_size, walkers, seed
    (1.0, 2, 1.0, 0.245, 4, 12, 8), (1.0, 2, 1.0, 0.245, 4, 8, 8), (2.0, 2, 1.0, 0.245, 5, 12, 8),
    (2.0, 2, 1.0, 0.245, 5, 8, 8)]


def check_cosines(tag):
    for c in COS:
        assert abs(c) > 1e-6 or c < -1e-3, (tag, c)
    kills = sum(1 for c in COS if c <= 0)
    del COS[:]
    return kills


def case_a(out, k, ecut, ne, rs, stack_size, fb_bound):
    beta, dt = 0.5, 0.05
    system = UEG({'nup': ne, 'ndown': ne, 'rs': rs, 'ecut': ecut, 'thermal': True, 'mu': 0.245}, verbose=False)
    trial = OneBody(system, beta, dt, verbose=False)
    qmc = dotdict({'dt': dt, 'nstblz': 10})
    prop = PlaneWave(system, trial, qmc, {'optimised': True, 'fb_bound': fb_bound}, verbose=False, lowrank=False)
    numpy.random.seed(7 + k)
    walker = ThermalWalker(system, trial, walker_opts={'stack_size': stack_size, 'low_rank': False}, verbose=False)
    nslice = int(round(beta / dt))
    assert walker.stack_size == stack_size and walker.num_slices == nslice
    pre = 'a%d_' % k
    out.update({pre + 'ecut': ecut, pre + 'nelec': ne, pre + 'rs': rs, pre + 'stack_size': stack_size,
                pre + 'fb_bound': fb_bound, pre + 'beta': beta, pre + 'dt': dt, pre + 'mu_system': float(system.mu), pre + 'mu': float(trial.mu),
                pre + 'dmat': numpy.array([trial.dmat[s].diagonal().real for s in range(2)]),
                pre + 'dmat_inv': numpy.array([trial.dmat_inv[s].diagonal().real for s in range(2)]),
                pre + 'BH1': numpy.array([prop.BH1[s].diagonal().real for s in range(2)]),
                pre + 'mf_shift': numpy.array(prop.mf_shift), pre + 'G0': walker.G.copy(), pre + 'M00': walker.M0.copy()})
    assert numpy.max(numpy.abs(trial.dmat[0] - numpy.diag(trial.dmat[0].diagonal()))) == 0.0
    assert numpy.max(numpy.abs(prop.BH1[0] - numpy.diag(prop.BH1[0].diagonal()))) < 1e-300
    seen = {}
    normal, bias = numpy.random.normal, prop.construct_force_bias_incore

    def rec_normal(*a):
        seen['xi'] = normal(*a)
        return seen['xi']

    def rec_bias(s, G):
        seen['xbar'] = bias(s, G)          # (the clip rescales this array in place)
        return seen['xbar']
    two_body = prop.two_body_propagator

    def rec_two_body(w, s, fb=True):
        r = two_body(w, s, fb)
        seen['cmf'], seen['cfb'] = r[0], r[1]
        return r
    numpy.random.normal, prop.construct_force_bias_incore, prop.two_body_propagator = rec_normal, rec_bias, rec_two_body
    rows = {n: [] for n in ('xi', 'xbar', 'cmf', 'cfb', 'G', 'M0', 'weight')}
    nclip = 0
    try:
        for ts in range(nslice):
            prop.propagate_walker(system, walker, ts, 0)
            nclip += int(numpy.sum(numpy.abs(numpy.abs(seen['xbar']) - 1.0) < 1e-14))
            for n in ('xi', 'xbar', 'cmf', 'cfb'):
                rows[n].append(numpy.array(seen[n]))
            rows['G'].append(walker.G.copy())
            rows['M0'].append(numpy.array(walker.M0))
            rows['weight'].append(float(numpy.real(walker.weight)))
    finally:
        numpy.random.normal = normal
    assert walker.stack.time_slice == nslice                       # ran to the end
    assert rows['weight'][-1] > 0
    kills = check_cosines(pre)
    E = numpy.array(walker.local_energy(system))
    nav = complex(particle_number(one_rdm_from_G(walker.G)))
    out.update({pre + n: numpy.array(v) for n, v in rows.items()})
    out.update({pre + 'energy': E, pre + 'nav': nav, pre + 'nclip': nclip, pre + 'kills': kills})


def case_b(out, k, ecut, ne, beta, mu, stack_size, nwalkers, seed):
    options = {'verbosity': 0, 'get_sha1': False,
               'qmc': {'timestep': 0.05, 'beta': beta, 'num_walkers': nwalkers, 'blocks': 2, 'pop_control_freq': 5,
                       'rng_seed': seed},
               'model': {'name': 'UEG', 'rs': 1.0, 'ecut': ecut, 'nup': ne, 'ndown': ne, 'mu': mu},
               'trial': {'name': 'one_body'},
               'walkers': {'stack_size': stack_size, 'low_rank': False},
               'propagator': {'optimised': True},
               'estimates': {'mixed': {}}}
    comm = type(mg.MPI.COMM_WORLD)()
    h5py._STORE.clear()
    afqmc = ThermalAFQMC(comm, options=options)
    walk = afqmc.walk
    nslice = afqmc.qmc.ntime_slices
    weights, combs = [], []
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
    out.update({pre + 'ecut': ecut, pre + 'nelec': ne, pre + 'beta': beta, pre + 'mu_system': mu, pre + 'dt': 0.05,
                pre + 'stack_size': int(walk.walkers[0].stack_size), pre + 'nwalkers': nwalkers, pre + 'seed': seed,
                pre + 'npop_control': int(afqmc.qmc.npop_control), pre + 'ntime_slices': int(nslice),
                pre + 'mu': float(afqmc.trial.mu), pre + 'blocks': blocks,
                pre + 'header': numpy.array(afqmc.estimators.estimators['mixed'].header),
                pre + 'weights': numpy.array(weights).reshape(2 * nslice, nwalkers),
                pre + 'comb_r': numpy.array([c[0] for c in combs]),
                pre + 'comb_weights': numpy.array([c[1] for c in combs]),
                pre + 'parent_ix': numpy.array([c[2] for c in combs]), pre + 'kills': kills})


def make_thermal_ueg():
    out = {}
    for k, case in enumerate(A_CASES):
        case_a(out, k, *case)
    for k, case in enumerate(B_CASES):
        case_b(out, k, *case)
    assert out['a4_nclip'] > 0, 'the clip case does not clip'
    assert max(out['a%d_nclip' % k] for k in range(4)) == 0
    mg.save('thermal_ueg.npz', out)
    assert os.path.getsize(os.path.join(mg.OUT, 'thermal_ueg.npz')) < 1000 * 1000


FIXTURES = [('thermal_ueg.npz', make_thermal_ueg)]


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
