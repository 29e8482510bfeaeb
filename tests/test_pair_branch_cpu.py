"""Pair-branch population control (walkers/handler.py:225-251,340-412) on the host: ``pair_branch_plan`` against the
events the genuine reference produced (tests/golden/pair_branch.npz), the known answer of the reference's own
walkers/tests/test_handler.py, the routing rule between ranks against a message-by-message restatement, and the
``Walkers`` option.  No GPU."""
import collections

import numpy
import pytest

from pauxy_amd import _lib as L
from pauxy_amd import systems, trial as trial_mod
from pauxy_amd.context import release_context
from pauxy_amd.walkers.handler import pair_branch_plan
from tests import dropin_checks, oracle_device


def events(d):
    for k, name in enumerate(d['event_names']):
        yield str(name), {key[len('ev%d_' % k):]: d[key] for key in d if key.startswith('ev%d_' % k)}


def scaled(w):
    """walkers/handler.py:230-246: total = sum(|w|) left to right, weight / (total / target)."""
    total = sum(numpy.abs(w))
    return w / (total / len(w)), total


def origins(n, pairs):
    org = numpy.arange(n)
    for c, k in pairs:
        org[k] = c
    return org


def test_plan_reproduces_every_recorded_event(golden):
    d = golden('pair_branch.npz')
    seen = []
    for name, ev in events(d):
        w, total = scaled(ev['w_in'])
        assert total == float(ev['total_weight'])
        new_w, mult, pairs, ndraws = pair_branch_plan(w, float(ev['min_weight']), float(ev['max_weight']), ev['draws'])
        assert ndraws == ev['draws'].size, name
        assert numpy.array_equal(new_w, ev['w_out']), name                    # bitwise
        assert numpy.array_equal(origins(len(w), pairs), ev['origin']), name
        assert mult.dtype == numpy.int32
        assert numpy.array_equal(mult, 1 + numpy.bincount([c for c, _ in pairs], minlength=len(w))
                                 - numpy.bincount([k for _, k in pairs], minlength=len(w))), name
        # unscaled_weight travels with the walker (the buffer of :400-410)
        assert numpy.array_equal(ev['w_in'][ev['origin']], ev['unscaled_out']), name
        assert abs(new_w.sum() - len(w)) < 1e-12 or (ev['w_in'] < 0).any(), name
        seen.append(name)
    assert seen == ['worked', 'odd11', 'two', 'three', 'none', 'max_only', 'bounds', 'small_cloned']


def test_plan_draws_from_a_callable_once_per_active_pair(golden):
    d = golden('pair_branch.npz')
    for name, ev in events(d):
        w, _ = scaled(ev['w_in'])
        numpy.random.seed(int(ev['seed']))
        new_w, _, _, ndraws = pair_branch_plan(w, float(ev['min_weight']), float(ev['max_weight']), numpy.random.rand)
        assert numpy.array_equal(new_w, ev['w_out']), name
        assert numpy.random.rand() == float(ev['next_draw']), name             # the stream is where the reference left it


def test_worked_example_of_the_issue(golden):
    ev = dict(events(golden('pair_branch.npz')))['worked']
    assert numpy.allclose(ev['draws'], [0.18026969, 0.01947524, 0.46321853, 0.72493393], rtol=0, atol=1e-8)
    assert list(ev['origin']) == [2, 1, 2, 4, 4, 6, 6, 7, 8, 10, 10, 11]
    assert ev['unscaled_out'][3] == -1.2 and ev['unscaled_out'][4] == -1.2
    assert ev['w_out'].sum() == pytest.approx(12.0, rel=1e-14)


HANDLER_W = numpy.array([0.001, 1.0148, 4.348, 1.2, 2.348, 4.4])          # walkers/tests/test_handler.py, two ranks of three


def test_known_answer_of_the_reference_s_handler_test():
    numpy.random.seed(7)
    new_w, mult, pairs, ndraws = pair_branch_plan(HANDLER_W, 0.1, 4.0, numpy.random.rand, 3)
    assert ndraws == 2 and list(mult) == [0, 0, 2, 1, 1, 2]
    assert sorted(pairs) == [(2, 1), (5, 0)]              # rank 0: slot 0 from rank 1, slot 1 from itself
    assert new_w[0] == new_w[5] == 0.5 * (0.001 + 4.4) and new_w[1] == new_w[2] == 0.5 * (1.0148 + 4.348)
    assert new_w[3] == 1.2 and new_w[4] == 2.348


def messages(weights, min_weight, max_weight, draws, per):
    """The reference's protocol, message by message: rank 0's table [a, mult, rank, partner rank] per walker; every rank
    posts its clones in local order to the partner's rank, every rank receives for its kills in local order from the
    partner's rank, and messages between two ranks match in posting order.  -> {destination slot: source walker}."""
    a = [abs(float(x)) for x in weights]
    n = len(a)
    order = sorted(range(n), key=lambda i: (a[i], i))
    table = [[a[i], 1, i // per, i // per] for i in range(n)]
    draws = list(draws)
    for p in range(n // 2):
        lo, hi = table[order[p]], table[order[n - 1 - p]]
        if not (lo[0] < min_weight or hi[0] > max_weight):
            break
        r = draws.pop(0)
        cl, ki = (hi, lo) if r < hi[0] / (lo[0] + hi[0]) else (lo, hi)
        cl[0], cl[1], cl[3], ki[1], ki[3] = 0.5 * (lo[0] + hi[0]), 2, ki[2], 0, cl[2]
        ki[0] = 0.0
    wire = collections.defaultdict(collections.deque)
    for i in range(n):
        if table[i][1] == 2:
            wire[(i // per, table[i][3])].append((i, table[i][0]))
    landed = {}
    for i in range(n):
        if table[i][1] == 0:
            landed[i] = wire[(table[i][3], i // per)].popleft()
    assert not any(wire.values())
    return landed, table


def crowd(seed, n):
    rng = numpy.random.RandomState(seed)
    w = rng.choice([0.01, 0.05, 1.0, 1.0, 5.0, 8.0], n) * (0.5 + rng.rand(n))
    w[::5] *= -1.0
    w[3] = w[7]                                           # an exact tie
    return w, rng.rand(n // 2)


@pytest.mark.parametrize('seed', range(6))
def test_routing_between_three_ranks_is_the_message_order(seed):
    w, u = crowd(seed, 18)
    w, _ = scaled(w)
    new_w, mult, pairs, ndraws = pair_branch_plan(w, 0.1, 4.0, u, 6)
    landed, table = messages(w, 0.1, 4.0, u, 6)
    assert ndraws >= 3 and any(c // 6 != k // 6 for c, k in pairs), 'the case must move walkers between ranks'
    assert {k: c for c, k in pairs} == {k: src for k, (src, _) in landed.items()}
    assert list(mult) == [row[1] for row in table]
    for k, (src, wt) in landed.items():
        assert new_w[k] == wt == new_w[src]
    keep = [i for i in range(18) if mult[i] == 1]
    assert numpy.array_equal(new_w[keep], w[keep])        # signed, untouched
    # the one-rank result over the same weights: another placement, the same population
    w1, mult1, pairs1, nd1 = pair_branch_plan(w, 0.1, 4.0, u)
    assert nd1 == ndraws and numpy.array_equal(mult1, mult)
    clones = numpy.where(mult == 2)[0].tolist()
    kills = numpy.where(mult == 0)[0].tolist()
    assert pairs1 == list(zip(clones, kills))
    assert sorted(zip(origins(18, pairs1).tolist(), w1.tolist())) == sorted(zip(origins(18, pairs).tolist(), new_w.tolist()))


def small_hubbard(golden):
    d = golden('traj_hubbard_c1.npz')
    s = systems.Hubbard(4, 4, 8, 8, float(d['U']))
    return s, trial_mod.SingleDetTrial(s, d['psi'], name='UHF')


def shell(golden, walker_opts):
    s, t = small_hubbard(golden)
    sh, comm = dropin_checks.build_shell(s, t, {'timestep': 0.01, 'num_steps': 10, 'blocks': 1, 'num_walkers': 10},
                                         {'hubbard_stratonovich': 'continuous'}, {'mixed': {'energy_eval_freq': 1}},
                                         walker_opts)
    return sh, comm, s, t


def test_walkers_accepts_pair_branch_and_refuses_anything_else(golden, monkeypatch):
    oracle_device.install(monkeypatch)
    sh, comm, s, t = shell(golden, {'population_control': 'pair_branch', 'min_weight': 0.5, 'max_weight': 2.0})
    assert (sh.psi.pcont_method, sh.psi.min_weight, sh.psi.max_weight) == ('pair_branch', 0.5, 2.0)
    release_context(s, t)
    with pytest.raises(NotImplementedError):
        shell(golden, {'population_control': 'nonsense'})
    release_context(s, t)


def test_device_comm_with_pair_branch_on_several_ranks_is_refused_at_construction(golden, monkeypatch):
    oracle_device.install(monkeypatch)

    class TwoRanks(dropin_checks.FakeComm):
        size = 2
    monkeypatch.setattr(dropin_checks, 'FakeComm', TwoRanks)
    with pytest.raises(NotImplementedError, match='device communicator does the comb only'):
        shell(golden, {'population_control': 'pair_branch', 'device_comm': 'ipc'})
    s, t = small_hubbard(golden)
    release_context(s, t)


def test_pop_control_leaves_the_host_stream_where_the_reference_does(golden, monkeypatch):
    """Walkers.pop_control over a stand-in device whose event is the host plan: nw // 2 uniforms go to the device, the
    stream ends ndraws past its start, total weight and mult are kept; fetch=False advances it by nw // 2."""
    oracle_device.install(monkeypatch)
    ev = dict(events(golden('pair_branch.npz')))['odd11']

    def popcontrol_pair_branch(self, u, target, min_weight, max_weight, fetch=True):
        assert len(u) == self.nw // 2
        w = numpy.array([x['weight'] for x in self._w])
        total = sum(numpy.abs(w))
        new_w, mult, pairs, nd = pair_branch_plan(w / (total / target), min_weight, max_weight, u)
        for c, k in pairs:
            self.copy_walker(c, k)
        for i, x in enumerate(self._w):
            x['weight'] = new_w[i]
        return (mult, nd, float(total)) if fetch else (None, None, None)
    monkeypatch.setattr(oracle_device.OracleDevice, 'popcontrol_pair_branch', popcontrol_pair_branch, raising=False)
    s, t = small_hubbard(golden)
    sh, comm = dropin_checks.build_shell(s, t, {'timestep': 0.01, 'num_steps': 10, 'blocks': 1, 'num_walkers': 11},
                                         {'hubbard_stratonovich': 'continuous'}, {'mixed': {'energy_eval_freq': 1}},
                                         {'population_control': 'pair_branch'})
    psi = sh.psi
    psi.dev.set(L.F_WEIGHT, ev['w_in'])
    psi._invalidate()
    numpy.random.seed(int(ev['seed']))
    psi.pop_control(comm)
    assert numpy.random.rand() == float(ev['next_draw'])
    assert numpy.array_equal(psi.dev.get(L.F_WEIGHT), ev['w_out'])
    assert psi.total_weight == float(ev['total_weight']) and psi.walkers[3].total_weight == psi.total_weight
    assert (psi.last_parent_ix == 2).sum() == ev['draws'].size
    numpy.random.seed(3)
    psi.pop_control(comm, fetch=False)
    numpy.random.seed(3)
    numpy.random.rand(11 // 2)
    after = numpy.random.get_state()[2]
    numpy.random.seed(3)
    psi.dev.set(L.F_WEIGHT, ev['w_in'])
    psi.pop_control(comm, fetch=False)
    assert numpy.random.get_state()[2] == after
    release_context(s, t)
