#!/usr/bin/env python3
"""Golden fixture for the finite-temperature Hubbard path, from the genuine reference (qmc/thermal_afqmc.py,
thermal_propagation/hubbard.py, walkers/thermal.py, trial_density_matrices/onebody.py).

  thermal_hubbard.npz
    a_*   the reference's own unit-test case (thermal_propagation/tests/test_propagation.py, test_hubbard): Hubbard
          4 x 4, U = 4, mu = 1, 7 + 7 electrons, beta = 2, dt = 0.05, nstblz = 10, OneBody trial; one ThermalWalker each
          at stack_size 1 and 10 driven by ThermalDiscrete.propagate_walker with the uniforms of seed 7: the trial's
          mu / dmat / stack_size, the propagator's auxf / BH1, the uniforms, the fields chosen, G and the weight after
          every slice, the final (E, T, V) and nav.  (The unit test divides the weight by 1e6 after every slice; so
          does this record: a_weight_scale.)
    b_*   ThermalAFQMC on the same model with beta = 1, 6 walkers, walkers: {stack_size: 5}, pop_control_freq 5,
          two paths (blocks: 2), seed 7: every uniform in the order drawn (site uniforms and the comb's r, with the
          positions of the r's), the estimator rows (with the Nav column; the Time column zeroed) and the
          stabilisation period the walker handler settled on.
    min_margin   the smallest |u - p_0 / norm| over every recorded decision: no decision is within 1e-6 of its
          threshold (asserted here), so a rounding difference cannot flip a field.

Uses the import recipe of make_golden.py (which it imports and does not change); runs only where the reference is
available.

Usage:  python tests/golden/make_golden_thermal.py            (writes tests/golden/thermal_hubbard.npz)
        python tests/golden/make_golden_thermal.py --check    regenerate into a scratch directory and compare
"""
import os
import shutil
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg                                                 # noqa: E402  (prepares the reference)
from make_golden import Hubbard, dotdict, h5py                           # noqa: E402
from pauxy.trial_density_matrices.onebody import OneBody                 # noqa: E402
from pauxy.thermal_propagation.hubbard import ThermalDiscrete            # noqa: E402
from pauxy.walkers.thermal import ThermalWalker                          # noqa: E402
from pauxy.estimators.thermal import one_rdm_from_G, particle_number     # noqa: E402
from pauxy.qmc.thermal_afqmc import ThermalAFQMC                         # noqa: E402

MODEL = {'nx': 4, 'ny': 4, 'U': 4, 'mu': 1.0, 'nup': 7, 'ndown': 7}
MARGIN = [numpy.inf]


class Stream(object):
    """numpy.random.random with every draw recorded."""

    def __init__(self):
        self.drawn = []
        self._random = numpy.random.random

    def __enter__(self):
        def random(*a):
            x = self._random(*a)
            self.drawn.append(float(x))
            return x
        numpy.random.random = random
        return self

    def __exit__(self, *a):
        numpy.random.random = self._random
        return False


def watch_decisions(prop):
    """Wraps calculate_overlap_ratio so that the threshold of every decision is known: the next uniform drawn is
    compared with it."""
    inner = prop.calculate_overlap_ratio
    state = {}

    def ratio(walker, i):
        probs = inner(walker, i)
        p = numpy.maximum(probs.real, [0, 0])
        state['thr'] = p[0] / sum(p) if sum(p) > 0 else None
        return probs
    prop.calculate_overlap_ratio = ratio
    return state


def watch_margins(prop, stream_of):
    """Every site decision of ``prop`` from now on: the uniform drawn for it (the last of the current Stream) against
    its threshold.  The rank-1 update is the first call after the draw, and it happens only when a decision was made."""
    state = watch_decisions(prop)
    update = prop.update_greens_function

    def update_and_check(walker, i, xi):
        MARGIN[0] = min(MARGIN[0], abs(stream_of().drawn[-1] - state['thr']))
        return update(walker, i, xi)
    prop.update_greens_function = update_and_check


def fields_of(BV, auxf):
    """The fields a slice chose, read back from BV[0, i] == auxf[x, 0]."""
    x = numpy.where(BV[0] == auxf[0, 0], 0, 1)
    assert numpy.all(BV[0] == auxf[x, 0]) and numpy.all(BV[1] == auxf[x, 1])
    return x.astype(numpy.int32)


def case_a(out):
    system = Hubbard(dict(MODEL), verbose=False)
    beta, dt = 2.0, 0.05
    nslice = int(round(beta / dt))
    trial = OneBody(system, beta, dt)
    qmc = dotdict({'dt': dt, 'nstblz': 10})
    prop = ThermalDiscrete(system, trial, qmc, verbose=False)
    assert not numpy.iscomplexobj(prop.auxf) and not numpy.iscomplexobj(prop.BH1)
    out.update(a_T=system.T.real, a_U=float(system.U), a_mu_system=float(system.mu), a_beta=beta, a_dt=dt,
               a_nstblz=10, a_nelec=numpy.array([system.nup, system.ndown]), a_mu=float(trial.mu),
               a_dmat=numpy.array(trial.dmat.real), a_dmat_inv=numpy.array(trial.dmat_inv.real),
               a_trial_stack_size=int(trial.stack_size), a_num_slices=int(trial.num_slices),
               a_trial_nav=float(trial.nav), a_auxf=numpy.array(prop.auxf), a_BH1=numpy.array(prop.BH1),
               a_weight_scale=1.0e6, a_stack_sizes=numpy.array([1, 10]))
    cur = {}
    watch_margins(prop, lambda: cur['st'])
    for k, stack_size in enumerate((1, 10)):
        numpy.random.seed(7)
        walker = ThermalWalker(system, trial, walker_opts={'stack_size': stack_size, 'low_rank': False}, verbose=False)
        assert numpy.max(numpy.abs(walker.G.imag)) == 0.0
        G0 = walker.G.real.copy()
        Gs, ws, us, xs = [], [], [], []
        for ts in range(nslice):
            with Stream() as st:
                cur['st'] = st
                prop.propagate_walker(system, walker, ts, 0)
            assert len(st.drawn) == system.nbasis
            us.append(st.drawn)
            xs.append(fields_of(prop.BV, prop.auxf))
            walker.weight /= 1.0e6
            assert numpy.max(numpy.abs(walker.G.imag)) == 0.0
            Gs.append(walker.G.real.copy())
            ws.append(float(numpy.real(walker.weight)))
        E = numpy.array(walker.local_energy(system)).real
        nav = float(particle_number(one_rdm_from_G(walker.G)).real)
        out.update({'a%d_G0' % k: G0, 'a%d_G' % k: numpy.array(Gs), 'a%d_weight' % k: numpy.array(ws),
                    'a%d_u' % k: numpy.array(us), 'a%d_fields' % k: numpy.array(xs), 'a%d_energy' % k: E,
                    'a%d_nav' % k: nav})


def case_b(out):
    options = {'verbosity': 0, 'get_sha1': False,
               'qmc': {'timestep': 0.05, 'beta': 1.0, 'num_walkers': 6, 'blocks': 2, 'pop_control_freq': 5,
                       'rng_seed': 7},
               'model': dict(MODEL, name='Hubbard'),
               'trial': {'name': 'one_body'},
               'walkers': {'stack_size': 5},
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
    out['blocks'] = numpy.array([store[k] for k in keys])
    out['b_header'] = numpy.array(afqmc.estimators.estimators['mixed'].header)
    out.update(b_draws=numpy.array(st.drawn), b_r_pos=numpy.array(r_pos, dtype=numpy.int64), b_nwalkers=6,
               b_beta=1.0, b_dt=0.05, b_stack_size=int(walk.walkers[0].stack_size), b_nstblz=int(afqmc.qmc.nstblz),
               b_npop_control=int(afqmc.qmc.npop_control), b_paths=2, b_seed=7,
               b_mu=float(afqmc.trial.mu), b_dmat=numpy.array(afqmc.trial.dmat.real),
               b_auxf=numpy.array(afqmc.propagators.auxf), b_BH1=numpy.array(afqmc.propagators.BH1),
               b_ntime_slices=int(afqmc.qmc.ntime_slices))
    assert len(out['blocks']) == 3 and out['blocks'].shape[1] == 12, out['blocks'].shape
    assert len(r_pos) >= 2


def make_thermal():
    out = {}
    MARGIN[0] = numpy.inf
    case_a(out)
    case_b(out)
    assert MARGIN[0] > 1e-6, MARGIN[0]
    out['min_margin'] = float(MARGIN[0])
    mg.save('thermal_hubbard.npz', out)
    assert os.path.getsize(os.path.join(mg.OUT, 'thermal_hubbard.npz')) < 1000 * 1000


FIXTURES = [('thermal_hubbard.npz', make_thermal)]


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
