#!/usr/bin/env python3
"""Golden fixture for pair-branch population control, from the genuine reference (walkers/handler.py:225-251,340-412).

  pair_branch.npz
    ev<k>_*    single events of the reference's own Walkers.pop_control on a small Generic population whose walkers'
               phi are tagged with their index: inputs (weights, min_weight / max_weight, the uniforms it consumed) and
               outputs (weights, unscaled_weight, the slot every walker came from, the next uniform of the stream)
    t_*        a phaseless trajectory of the reference's Walkers + Continuous (Generic, M = 10, 3+3 electrons,
               12 walkers, 30 steps, re-orthogonalisation and population control every 5 steps, tightened bounds):
               the model, the fields and uniforms drawn (zeros for a dead walker, which the driver's loop does not
               propagate), and every step's weight / ot / hybrid_energy

The reference sends every cloned walker through its communicator even on one rank.  make_golden.py's communicator
stand-in keys its mailbox by tag alone -- and every pair-branch message of one rank carries the same tag -- so this
script hands the reference a communicator of its own with one FIFO queue per (destination, tag), which is what the
message matching of MPI amounts to.

Uses the import recipe of make_golden.py (which it imports and does not change); runs only where the reference is
available.

Usage:  python tests/golden/make_golden_pair_branch.py            (writes tests/golden/pair_branch.npz)
        python tests/golden/make_golden_pair_branch.py --check    regenerate into a scratch directory and compare
"""
import collections
import os
import shutil
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg                                                 # noqa: E402  (prepares the reference)
from make_golden import Generic, MultiSlater, Continuous, generate_hamiltonian, get_random_nomsd, dotdict  # noqa: E402
from pauxy.walkers.handler import Walkers                                # noqa: E402


class _Req(object):
    def wait(self):
        pass


class FifoComm(object):
    """One rank; point-to-point messages match in posting order per (destination, tag)."""
    rank, size = 0, 1

    def __init__(self):
        self.box = collections.defaultdict(collections.deque)

    def barrier(self):
        pass

    Barrier = barrier

    def Allgather(self, s, r):
        r[...] = numpy.asarray(s).reshape(r.shape)

    def gather(self, x, root=0):
        return [x]

    def scatter(self, x, root=0):
        return x[0]

    def bcast(self, x, root=0):
        return x

    def Isend(self, buf, dest=0, tag=0):
        self.box[(int(dest), float(tag))].append(numpy.array(buf, copy=True))
        return _Req()

    def Recv(self, buf, source=0, tag=0):
        buf[...] = self.box[(self.rank, float(tag))].popleft()

    def empty(self):
        return not any(self.box.values())


def small_generic(nmo=10, nelec=(3, 3), nchol=40):
    """generate_hamiltonian's system with its first ``nchol`` Cholesky vectors (a Hamiltonian as good as the full one
    for this purpose, and the recorded fields stay small)."""
    numpy.random.seed(7)
    h1e, chol, enuc, eri = generate_hamiltonian(nmo, nelec, cplx=False)
    chol = chol[:nchol]
    system = Generic(nelec=nelec, h1e=numpy.array([h1e, h1e]), chol=chol.reshape((-1, nmo * nmo)).T.copy(), ecore=enuc)
    trial = MultiSlater(system, get_random_nomsd(system, ndet=1, cplx=False))
    trial.half_rotate(system)
    trial.psi = trial.psi.astype(numpy.complex128)
    trial._rchol = trial._rchol.astype(numpy.complex128)
    trial.init = numpy.asarray(trial.init, dtype=numpy.complex128)
    trial.all_dets = trial.psi                      # [1, M, na+nb]: Walkers.__init__ replaces trial.psi by trial.psi[0]
    return system, trial, h1e, enuc


def population(system, trial, nw, opts):
    qmc = dotdict({'nwalkers': nw, 'ntot_walkers': nw, 'dt': 0.005, 'nstblz': 5})
    comm = FifoComm()
    trial.psi = trial.all_dets
    psi = Walkers(system, trial, qmc, walker_opts=dict(opts, population_control='pair_branch'), comm=comm)
    return psi, comm


class Stream(object):
    """numpy.random.rand with every draw recorded."""

    def __init__(self):
        self.drawn = []
        self._rand = numpy.random.rand

    def __enter__(self):
        def rand(*a):
            x = self._rand(*a)
            self.drawn.append(float(x))
            return x
        numpy.random.rand = rand
        return self

    def __exit__(self, *a):
        numpy.random.rand = self._rand
        return False


def one_event(system, trial, weights, min_weight, max_weight, seed):
    """Walker i carries phi = trial.init * (i + 1): the slot origins are read back from the tags."""
    nw = len(weights)
    psi, comm = population(system, trial, nw, {'min_weight': min_weight, 'max_weight': max_weight})
    for i, w in enumerate(psi.walkers):
        w.weight = float(weights[i])
        w.unscaled_weight = -7.0                       # (overwritten by the event)
        w.phi = trial.init * (i + 1.0)
    numpy.random.seed(seed)
    with Stream() as st:
        psi.pop_control(comm)
    assert comm.empty()
    origin = numpy.array([int(round((w.phi.ravel()[0] / trial.init.ravel()[0]).real)) - 1 for w in psi.walkers])
    for i, w in enumerate(psi.walkers):
        assert numpy.array_equal(w.phi, trial.init * (origin[i] + 1.0))
    return dict(w_in=numpy.array(weights, dtype=numpy.float64), min_weight=float(min_weight), max_weight=float(max_weight),
                seed=int(seed), draws=numpy.array(st.drawn, dtype=numpy.float64),
                w_out=numpy.array([w.weight for w in psi.walkers], dtype=numpy.float64),
                unscaled_out=numpy.array([w.unscaled_weight for w in psi.walkers], dtype=numpy.float64),
                origin=origin.astype(numpy.int32), next_draw=float(numpy.random.rand()),
                total_weight=float(psi.walkers[0].total_weight))


WORKED = [0.02, 1.0, 5.5, 0.05, -1.2, 0.05, 6.0, 0.9, 1.1, 0.03, 7.0, 1.0]


def small_cloned(ev):
    """True when some pair of the event cloned its LIGHT walker: a walker that was below the median weight got mult 2."""
    a = numpy.abs(ev['w_in'])
    order = numpy.argsort(a, kind='mergesort')
    light = set(order[:len(a) // 2].tolist())
    counts = numpy.bincount(ev['origin'], minlength=len(a))
    return any(counts[i] == 2 for i in light)


def make_events(system, trial, out):
    rng = numpy.random.RandomState(3)
    events = [
        ('worked', one_event(system, trial, WORKED, 0.1, 4.0, 11)),
        ('odd11', one_event(system, trial, numpy.concatenate([[0.01, 0.04, 9.0, -0.02, 6.5], rng.rand(6) + 0.5]), 0.1, 4.0, 5)),
        ('two', one_event(system, trial, [0.05, 2.5], 0.1, 4.0, 2)),
        ('three', one_event(system, trial, [1.4, -0.01, 1.3], 0.1, 4.0, 3)),
        ('none', one_event(system, trial, 0.8 + 0.4 * rng.rand(10), 0.1, 4.0, 4)),
        ('max_only', one_event(system, trial, numpy.concatenate([[40.0, 1.9, 38.0], 1.8 + 0.4 * rng.rand(7)]), 0.1, 4.0, 6)),
        ('bounds', one_event(system, trial, [0.3, 2.9, 1.0, 0.2, 1.05, 3.3, 0.95, 0.6, 1.0], 0.5, 2.0, 8)),
    ]
    d = dict(events)
    assert d['worked']['draws'].size == 4 and abs(d['worked']['draws'][0] - 0.18026969) < 1e-8
    assert list(d['worked']['origin']) == [2, 1, 2, 4, 4, 6, 6, 7, 8, 10, 10, 11]
    assert abs(d['worked']['w_out'].sum() - 12.0) < 1e-12 and d['worked']['unscaled_out'][3] == -1.2
    assert d['none']['draws'].size == 0 and list(d['none']['origin']) == list(range(10))
    assert d['max_only']['draws'].size == 2 and numpy.abs(d['max_only']['w_in']).min() / (numpy.abs(d['max_only']['w_in']).sum() / 10) > 0.1
    assert d['bounds']['draws'].size == 3            # (none of them under the default bounds)
    # a pair in which the light walker is cloned: the first seed (deterministic search) at which one occurs
    w_small = [0.09, 3.0, 1.0, 0.06, 2.2, 1.1, 0.9, 1.2]
    for seed in range(1000):
        ev = one_event(system, trial, w_small, 0.1, 1.5, seed)
        if small_cloned(ev):
            break
    assert small_cloned(ev), 'no seed below 1000 clones a light walker'
    events.append(('small_cloned', ev))
    out['event_names'] = numpy.array([n for n, _ in events])
    for k, (name, ev) in enumerate(events):
        for key, v in ev.items():
            out['ev%d_%s' % (k, key)] = v


def make_trajectory(system, trial, h1e, enuc, out, nw=12, nsteps=30, every=5, dt=0.05, bounds=(0.6, 1.6)):
    psi, comm = population(system, trial, nw, {'min_weight': bounds[0], 'max_weight': bounds[1]})
    qmc = dotdict({'dt': dt, 'nstblz': every})
    numpy.random.seed(8)
    prop = Continuous(system, trial, qmc, options={})
    assert not prop.free_projection
    K = system.nfields
    xi = numpy.zeros((nsteps, nw, K))
    out['t_phi0'] = numpy.array([w.phi for w in psi.walkers])
    out['t_ot0'] = numpy.array([w.ot for w in psi.walkers], dtype=numpy.complex128)
    rec = dict(weight=[], ot=[], ehyb=[], unscaled=[])
    draws, ndraws = [], []
    _normal = numpy.random.normal
    cur = {}

    def normal(*a, **k):
        x = _normal(*a, **k)
        xi[cur['step'], cur['iw']] = x
        return x

    eshift = 0.0
    numpy.random.normal = normal
    try:
        for step in range(1, nsteps + 1):
            if step % every == 0:
                psi.orthogonalise(trial, False)
            for iw, w in enumerate(psi.walkers):
                cur.update(step=step - 1, iw=iw)
                if abs(w.weight) > 1e-8:                       # the driver's test, qmc/afqmc.py:232
                    prop.propagate_walker(w, system, trial, eshift)
            if step % every == 0:
                with Stream() as st:
                    psi.pop_control(comm)
                assert comm.empty()
                draws.extend(st.drawn)
                ndraws.append(len(st.drawn))
            rec['weight'].append([w.weight for w in psi.walkers])
            rec['unscaled'].append([w.unscaled_weight for w in psi.walkers])
            rec['ot'].append([w.ot for w in psi.walkers])
            rec['ehyb'].append([w.hybrid_energy for w in psi.walkers])
    finally:
        numpy.random.normal = _normal
    assert sum(1 for n in ndraws if n > 0) >= 3, ndraws          # at least three events pair walkers
    out.update(t_h1e=h1e, t_chol=system.chol_vecs, t_ecore=enuc, t_nelec=numpy.array([system.nup, system.ndown]),
               t_rchol=trial._rchol, t_psi=trial.psi, t_BH1=prop.propagator.BH1, t_mf_shift=prop.propagator.mf_shift,
               t_dt=dt, t_every=every, t_min_weight=bounds[0], t_max_weight=bounds[1], t_eshift=eshift,
               t_xi=xi, t_u=numpy.array(draws, dtype=numpy.float64), t_ndraws=numpy.array(ndraws, dtype=numpy.int32),
               t_weight=numpy.array(rec['weight'], dtype=numpy.float64),
               t_unscaled_weight=numpy.array(rec['unscaled'], dtype=numpy.float64),
               t_ot=numpy.array(rec['ot'], dtype=numpy.complex128),
               t_hybrid_energy=numpy.array(rec['ehyb'], dtype=numpy.complex128))


def make_pair_branch():
    out = {}
    system, trial, h1e, enuc = small_generic()
    make_events(system, trial, out)
    system, trial, h1e, enuc = small_generic()
    make_trajectory(system, trial, h1e, enuc, out)
    mg.save('pair_branch.npz', out)
    assert os.path.getsize(os.path.join(mg.OUT, 'pair_branch.npz')) < 200 * 1024


FIXTURES = [('pair_branch.npz', make_pair_branch)]


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
