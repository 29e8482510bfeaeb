"""The decision branches of the phaseless constraint where the step closes as the TAIL of the fused propagator's launch
(prop_fused_kernel<false, 7, true, MUL3>: k_fused.hip, greens_small.h, weight_update.h) -- the launch every step of the
batched driver takes in the shape class.  The tail evaluates the Green's function of every walker, live or not, and its
weight update decides: the phase kill, both sides of the hybrid-energy bound, infinite and vanishing importance functions,
the cap behind a kill, the parked and the dead walkers it must leave alone, the counters, the estimator terms that ride on it.

The populations are the ``tail-*`` cases of tests/constraint_cases.py (checked on the reference alone in
tests/test_constraint_cases_cpu.py), the handle is made ready as tests/test_gpu_constraint_edges.py does, and two steps are
taken on each route to the tail:

  announced   mode 2, scope 0   estimates_fuse_next(); propagate(x, eshift)
  every-step  mode 2, scope 1   propagate(x, eshift)
  split       mode 2, scope 1   propagate_begin(x); estimates_fuse_next(); propagate_finish(eshift)   (weight_kernel decides)
  bitwise     mode 1, scope 1   propagate(x, eshift), against mode 0 in scope 0 (the two launches), every bit

After each step EVERY walker is held to the oracle by test_gpu_constraint_edges.check_step with its tolerances (continuous
values to 1e-9, decisions exactly); each route asserts the launches it ran, so a route that fell back to two launches fails
here.  ``tail-bp`` carries a back-propagation window: its steps must not fuse in any scope.  Each (case, mode, scope, way of
stepping) runs once and is shared by the tests below, unchanged.  Run with -s for the largest differences per (case, route)."""
import functools

import numpy
import pytest

from oracle import afqmc_ref as ref
from pauxy_amd import _lib as L
from tests import constraint_cases as cc
from tests.helpers import make_device
from tests.test_gpu_constraint_edges import EST, TOL, check_step, load_case, run_case
from tests.test_gpu_step_fusion import launches, same_bits
from tests.test_gpu_traj import close

pytestmark = pytest.mark.gpu
# route -> (mode, scope, how a step is taken)
ROUTES = {'announced': (2, 0, 'announced'), 'every-step': (2, 1, 'plain'), 'split': (2, 1, 'split'),
          'bitwise': (1, 1, 'plain')}
ORACLE_ROUTES = ('announced', 'every-step', 'split')
STATE = (L.F_PHI, L.F_WEIGHT, L.F_OT, L.F_HYBRID_ENERGY, L.F_ELOC, L.F_PHASE)
FIELDS = STATE + (L.F_XBAR, L.F_XSHIFTED)
BITWISE = (L.F_PHI, L.F_WEIGHT, L.F_OT, L.F_HYBRID_ENERGY, L.F_PHASE, L.F_XBAR, L.F_XSHIFTED)
RIDING = [ref.EST[k] for k in ('uweight', 'weight', 'ehyb', 'ovlp')]


@functools.lru_cache(maxsize=None)
def riding_sums(name):
    """What the estimator terms riding on the two steps must add up to: estimators/mixed.py:211-225 without the energy, over
    ALL walkers (dead, parked, killed and capped ones too) as each step leaves them.  The two steps of cc.run_oracle restated
    (that one keeps the walkers of the second step only); they end where its verdicts do."""
    run = cc.run_oracle(name)
    model, phis, weights, xi, eshift, extra = run['case']
    walkers = cc.new_walkers(model, phis, weights, extra['ehyb0'])
    for w, e in zip(walkers, extra['ehyb0']):
        w['eloc'] = complex(e)
    est = numpy.zeros(10, dtype=numpy.complex128)
    for x in (xi, extra['xi2']):
        cc.oracle_step(model, walkers, x, eshift, extra['hybrid'], extra['cap'])
        ref.mixed_update(model, est, walkers, 1, 2)
    last = run['verdicts'][-1]
    assert all(w['weight'] == v['weight'] and w['ot'] == v['ot'] for w, v in zip(walkers, last))
    est.setflags(write=False)
    return est


@functools.lru_cache(maxsize=None)
def device_run(name, mode, scope, how):
    """Two steps of a case -> the walkers ahead of the first; per step the walker fields, afq_counters_ext (reset behind each
    step) and the launch trace; ``riding``: the estimator sums behind the second step with no update of their own (announced
    and split steps); ``estimates``: the block estimates with the energy over what the second step left (plain steps)."""
    run = cc.run_oracle(name)
    model, phis, weights, xi, eshift, extra = run['case']
    dev = make_device(model, len(weights), hybrid=extra['hybrid'])
    try:
        load_case(dev, run)
        dev.set_step_fusion(mode)
        dev.set_step_fusion_scope(scope)
        out = dict(before={f: dev.get(f) for f in STATE}, steps=[])
        for x in (xi, extra['xi2']):
            x = None if extra['philox'] is not None else x
            dev.launch_trace(True)
            if how == 'announced':
                dev.estimates_fuse_next()
                dev.propagate(x, eshift)
            elif how == 'plain':
                dev.propagate(x, eshift)
            else:
                dev.propagate_begin(x)
                dev.estimates_fuse_next()
                dev.propagate_finish(eshift)
            trace = dev.launch_trace_get()
            dev.launch_trace(False)
            out['steps'].append(dict(fields={f: dev.get(f) for f in FIELDS}, counters=dev.counters(reset=True, n=8),
                                     trace=trace))
        if how == 'plain':
            dev.estimates_update(True)
            out['estimates'] = dev.estimates_get(zero=True)
        else:
            out['riding'] = dev.estimates_get()
        return out
    finally:
        dev.close()


class Recorded(object):
    """What check_step reads off a handle, as device_run recorded it behind one step."""

    def __init__(self, step):
        self.step = step

    def get(self, field):
        return self.step['fields'][field]

    def counters(self, reset=False, n=4):
        return self.step['counters'][:n]


def worst(got, verdicts, field, key):
    """Largest device-to-oracle difference of a field over the propagated walkers, in the measure of ``close``."""
    return max([float(numpy.max(numpy.abs(got[field][i] - v[key]))) / max(1.0, float(numpy.max(numpy.abs(v[key]))))
                for i, v in enumerate(verdicts) if v['live']], default=0.0)


def counts(r, mode):
    tail = 'prop_fused_kernel<false, 7, true, %s>' % ('true' if mode == 2 else 'false')
    return dict(props=[launches(s['trace'], 'prop_fused_kernel') for s in r['steps']],
                tails=[launches(s['trace'], tail) for s in r['steps']],
                greens=[launches(s['trace'], 'greens_small_kernel') for s in r['steps']],
                weight=[sum(n for k, (n, _ms) in s['trace'].items() if k == 'weight_kernel') for s in r['steps']])


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", cc.TAIL_FUSING)
def test_route_runs_the_tail(name, route):
    """Per step exactly one propagator launch and it is the one with the tail (of the body the mode names); a Green's function
    launch ahead of the first step only (nothing is cached there); weight_kernel once per split step and nowhere else."""
    mode, scope, how = ROUTES[route]
    c = counts(device_run(name, mode, scope, how), mode)
    split = 1 if how == 'split' else 0
    assert c == dict(props=[1, 1], tails=[1, 1], greens=[1, 0], weight=[split, split]), (name, route, c)


@pytest.mark.parametrize("route", ORACLE_ROUTES)
@pytest.mark.parametrize("name", cc.TAIL_FUSING)
def test_tail_decisions_against_the_oracle(name, route):
    """Every walker behind each of the two steps against the oracle's verdict: both counters exactly, weights of exactly 0,
    bounded energies on the bound, walkers that are not propagated -- dead from the start, parked at 5e-9, killed by the first
    step -- bit for bit in phi, weight, overlap, energies and phase although the tail evaluated their Green's functions.
    every-step: the block estimates with the energy, from the per-spin Ghalf the tail stored; announced and split: the sums
    that rode on the two weight updates, over all walkers."""
    mode, scope, how = ROUTES[route]
    run = cc.run_oracle(name)
    model, phis, weights, xi, eshift, extra = run['case']
    r = device_run(name, mode, scope, how)
    before, closed_steps = r['before'], 0
    diff = dict(phi=0.0, weight=0.0, ot=0.0, ehyb=0.0)
    for step, verdicts in zip(r['steps'], run['verdicts']):
        for k, f, key in (('phi', L.F_PHI, 'phi'), ('weight', L.F_WEIGHT, 'weight'), ('ot', L.F_OT, 'ot'),
                          ('ehyb', L.F_HYBRID_ENERGY, 'hybrid_energy')):
            diff[k] = max(diff[k], worst(step['fields'], verdicts, f, key))
    c = counts(r, mode)
    print("\n%s %s: largest difference from the oracle phi %.1e weight %.1e ot %.1e ehyb %.1e | launches per step: "
          "propagator with tail %s, greens_small_kernel %s, weight_kernel %s"
          % (name, route, diff['phi'], diff['weight'], diff['ot'], diff['ehyb'], c['tails'], c['greens'], c['weight']))
    for step, verdicts in zip(r['steps'], run['verdicts']):
        before, counters = check_step(Recorded(step), model, eshift, extra, verdicts, before)
        closed_steps += int(counters[3])
    # a walker no step propagated has no force bias and no shifted fields: its rows read back as allocated, zeros
    never = [i for i in range(len(weights)) if not any(vs[i]['live'] for vs in run['verdicts'])]
    assert len(never) >= 2
    for f in (L.F_XBAR, L.F_XSHIFTED):
        assert not numpy.any(r['steps'][-1]['fields'][f][never]), (name, route, f)
    if how == 'plain':
        close(r['estimates'][EST], run['estimates'][EST], TOL)
        if extra['closed_deal']:
            assert closed_steps > 0                     # (the closed-shell deal of the fused propagator took them)
    else:
        close(r['riding'][RIDING], riding_sums(name)[RIDING], TOL)


@pytest.mark.parametrize("name", cc.TAIL_FUSING)
def test_tail_behind_the_unchanged_body_is_bit_for_bit(name):
    """Mode 1 in scope 1 against mode 0 in scope 0 (the two launches test_gpu_constraint_edges holds to the oracle): walkers,
    weights, overlaps, hybrid energies, phases, force bias and shifted fields, the counters of both bounds and of the
    closed-shell deals, behind each step, and the block estimates: every bit."""
    two, one = device_run(name, 0, 0, 'plain'), device_run(name, 1, 1, 'plain')
    for n, (a, b) in enumerate(zip(two['steps'], one['steps'])):
        for f in BITWISE:
            assert same_bits(a['fields'][f], b['fields'][f]), (name, n, f)
        assert list(a['counters'][[0, 1, 3, 5]]) == list(b['counters'][[0, 1, 3, 5]]), (name, n)
    assert same_bits(two['estimates'], one['estimates'])


def test_steps_with_a_window_do_not_fuse():
    """``tail-bp`` in mode 2 and scope 1: the shape and the population of ``tail-100-25`` with a back-propagation window of
    two steps.  No launch with the tail (the case's ``absent``), every walker against the oracle after each step, and the
    recorded steps and the window's estimate as the two launches leave them."""
    assert 'prop_fused_kernel<false, 7, true' in cc.CASES['tail-bp']['absent'] and cc.CASES['tail-bp']['bp'] == 2
    run_case('tail-bp', fusion=(2, 1))
