"""The mode-2 tail's overlap matrix and inverse under the resident body's closing pass (afq_set_step_tail_overlap,
k_fused_closed.h): O = (psi^H B) S from the Taylor sum in LDS, multiplied by the eight waves ahead of the closing one-body pass
and inverted by wave 7 while waves 0-6 run that pass; the tail starts at O^-1 phi^T.

Shapes: the corners of the class, (M, n) = (97, 17), (100, 25), (104, 32), K = 8 fields, order 1, 3 and 6 (the Taylor sum ends
in either image of T).  Population: closed walkers, one open-shell walker (beta block perturbed: streamed body, old tail) and
one of weight zero (no body, old tail) in the same launch.  33 walkers, not fewer: the step's Green's function rides on the
propagator only where the force bias contracts the spin sum (k_fb_use_sum: more than 32 walkers), so a smaller population
never launches the kernel under test.  Procedure (scope 1, as the batched driver sets it): an announced step, an unannounced
one, a split begin / finish step announced between its halves, an announced step; the fields are the device's own Philox
draws, restated on the host for the oracle.  Tolerances are test_gpu_step_fusion's: 1e-10 per step taken, relative to the
largest element (tests.test_gpu_sizes.close), twice that between two device forms that are each held to the oracle.
Each (shape, order, mode, switch) runs once and is shared by the tests below, unchanged."""
import ctypes
import functools

import numpy
import pytest

from oracle import afqmc_ref as ref
from pauxy_amd import _lib as L
from tests.helpers import make_device
from tests.philox_ref import device_normals_fast
from tests.test_gpu_sizes import build, close
from tests.test_gpu_step_fusion import ESHIFT, SEED, launches, same_bits

K, NW = 8, 33
SHAPES = [(97, 17), (100, 25), (104, 32)]
ORDERS = [1, 3, 6]
KINDS = ('announced', 'unannounced', 'split', 'announced')
OPEN, DEAD = 1, 4
WALKER_FIELDS = (L.F_PHI, L.F_WEIGHT, L.F_OT, L.F_HYBRID_ENERGY, L.F_PHASE, L.F_XBAR)
TOL = 1e-10


@functools.lru_cache(maxsize=None)
def population(M, N, order, dt=0.01):
    model, rng = build(M, K, N, N, False, seed=31, dt=dt)
    model.exp_order = order
    assert numpy.array_equal(model.BH1[0], model.BH1[1]) and numpy.abs(model.BH1.imag).max() == 0.0
    half = model.psi[None, :, :N] + 0.1 * (rng.rand(NW, M, N) + 1j * rng.rand(NW, M, N))
    phis = numpy.concatenate([half, half], axis=2)
    phis[OPEN, :, N:] += 0.05 * (rng.rand(M, N) + 1j * rng.rand(M, N))
    w0 = numpy.ones(NW)
    w0[DEAD] = 0.0
    ot = numpy.array([ref.calc_overlap(p, model.psi, N, N) for p in phis])
    for a in (phis, w0, ot):
        a.setflags(write=False)
    return dict(model=model, phis=phis, w0=w0, ot=ot)


def clipped_force_bias(model, phi):
    _ovlp, ghalf, G = model.greens(phi)
    xbar = numpy.array(model.force_bias(ghalf, G), dtype=numpy.complex128)
    big = numpy.abs(xbar) > 1.0
    xbar[big] /= numpy.abs(xbar[big])
    return xbar


def oracle_steps(model, walkers, live, first_counter, nsteps):
    """nsteps oracle steps on the device's fields -> per step phi, weight, overlap, hybrid energy, the force bias the step
    used and the per-spin Ghalf it leaves."""
    N = model.na
    want = []
    for c in range(first_counter, first_counter + nsteps):
        xi = device_normals_fast(NW * K, SEED[0], SEED[1], c).reshape(NW, K)
        xbar = [clipped_force_bias(model, w['phi']) if live[i] else None for i, w in enumerate(walkers)]
        for i in range(NW):
            if live[i]:
                ref.propagate_walker_phaseless(model, walkers[i], xi[i], ESHIFT)
        ghalf = [numpy.concatenate(ref.greens_function(w['phi'], model.psi, N, N)[1], axis=0) if live[i] else None
                 for i, w in enumerate(walkers)]
        want.append(dict(phi=[numpy.array(w['phi']) for w in walkers], weight=[w['weight'] for w in walkers],
                         ot=[w['ot'] for w in walkers], ehyb=[w['hybrid_energy'] for w in walkers], xbar=xbar, ghalf=ghalf))
    return want


@functools.lru_cache(maxsize=None)
def oracle(M, N, order):
    case = population(M, N, order)
    walkers = [ref.new_walker(case['model'], case['phis'][i]) for i in range(NW)]
    return oracle_steps(case['model'], walkers, case['w0'] != 0.0, 0, len(KINDS))


def one_step(dev, how):
    dev.launch_trace(True)
    if how == 'announced':
        dev.estimates_fuse_next()
        dev.propagate(None, ESHIFT)
    elif how == 'unannounced':
        dev.propagate(None, ESHIFT)
    else:
        dev.propagate_begin(None)
        dev.estimates_fuse_next()
        dev.propagate_finish(ESHIFT)
    trace = dev.launch_trace_get()
    dev.launch_trace(False)
    counted = dev.counters(n=9)
    out = dict(fields={f: dev.get(f) for f in WALKER_FIELDS}, closed_prop=int(counted[3]), closed_greens=int(counted[5]),
               early=int(counted[8]), trace=trace)
    if how == 'unannounced':
        dev.launch_trace(True)
        out['ghalf'] = dev.get(L.F_GHALF)
        out['ghalf_trace'] = dev.launch_trace_get()
        dev.launch_trace(False)
    return out


def start(case, mode, on, model=None):
    dev = make_device(model or case['model'], NW)
    dev.set_step_fusion(mode)
    dev.set_step_fusion_scope(1)
    dev.set_step_tail_overlap(on)
    dev.rng_seed(*SEED)
    dev.set(L.F_PHI, case['phis'])
    dev.set(L.F_WEIGHT, case['w0'])
    dev.set(L.F_OT, case['ot'])
    dev.counters(reset=True, n=9)
    return dev


@functools.lru_cache(maxsize=None)
def run(M, N, order, mode, on):
    dev = start(population(M, N, order), mode, on)
    try:
        out = dict(steps=[one_step(dev, how) for how in KINDS])
        out['estimates'] = dev.estimates_get()
        return out
    finally:
        dev.close()


def check_against(step_out, want, case, tol, N):
    """One step's device fields against the oracle's; the zero-weight walker untouched."""
    f = step_out['fields']
    for i in range(NW):
        if case['w0'][i] == 0.0:
            assert numpy.array_equal(f[L.F_PHI][i], case['phis'][i]) and f[L.F_WEIGHT][i] == 0.0
            continue
        close(f[L.F_PHI][i], want['phi'][i], tol)
        close(f[L.F_WEIGHT][i], want['weight'][i], tol)
        close(f[L.F_OT][i], want['ot'][i], tol)
        close(f[L.F_HYBRID_ENERGY][i], want['ehyb'][i], tol)
        close(f[L.F_XBAR][i], want['xbar'][i], tol)
        assert numpy.array_equal(f[L.F_PHI][i, :, :N], f[L.F_PHI][i, :, N:]) == (i != OPEN), i
        if 'ghalf' in step_out:
            close(step_out['ghalf'][i].reshape(2 * N, -1), want['ghalf'][i], tol)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("on", [1, 0])
def test_every_kind_of_step_against_the_oracle(M, N, order, on):
    """Switch on and off: phi, overlap, weight, hybrid energy, the force bias each step made of the spin sum the step before
    left, the per-spin Ghalf the unannounced step's tail stores (fetching it launches nothing) and the counters, on each of
    the four steps; the estimator sums against the two-launch route's."""
    case, want = population(M, N, order), oracle(M, N, order)
    got, two = run(M, N, order, 2, on), run(M, N, order, 0, 0)
    live_closed = NW - 2
    for step, s in enumerate(got['steps']):
        check_against(s, want[step], case, TOL * (step + 1), N)
        assert s['closed_prop'] == live_closed * (step + 1)
        assert (s['closed_prop'], s['closed_greens']) == (two['steps'][step]['closed_prop'], two['steps'][step]['closed_greens'])
        assert s['early'] == (live_closed * (step + 1) if on else 0), (step, s['early'])
    assert launches(got['steps'][1]['ghalf_trace'], 'greens_small_kernel') == 0
    close(got['estimates'], two['estimates'], 2.0 * TOL * len(KINDS))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_switch_moves_nothing_but_the_resident_walkers_overlap(M, N, order):
    """On against off.  The propagated walker itself does not depend on the switch -- B S is made by the same statements -- so
    the first step's phi and force bias are the same bits for every walker; the open-shell and the zero-weight walker, which
    never take the resident body, keep every bit of every field on every step; the closed walkers' overlaps differ by the
    rounding of (psi^H B) S against psi^H (B S), within twice the oracle's tolerance.  Off is the launch of before: a second
    handle repeats it bit for bit, the path counter stays at zero."""
    on, off = run(M, N, order, 2, 1), run(M, N, order, 2, 0)
    assert same_bits(on['steps'][0]['fields'][L.F_PHI], off['steps'][0]['fields'][L.F_PHI])
    assert same_bits(on['steps'][0]['fields'][L.F_XBAR], off['steps'][0]['fields'][L.F_XBAR])
    for step, (a, b) in enumerate(zip(on['steps'], off['steps'])):
        for f in WALKER_FIELDS:
            for i in (OPEN, DEAD):
                assert same_bits(a['fields'][f][i], b['fields'][f][i]), (step, f, i)
            close(a['fields'][f], b['fields'][f], 2.0 * TOL * (step + 1))
        assert b['early'] == 0
    for i in (OPEN, DEAD):
        assert same_bits(on['steps'][1]['ghalf'][i], off['steps'][1]['ghalf'][i])
    dev = start(population(M, N, order), 2, 0)
    try:
        again = [one_step(dev, how) for how in KINDS]
    finally:
        dev.close()
    for a, b in zip(again, off['steps']):
        for f in WALKER_FIELDS:
            assert same_bits(a['fields'][f], b['fields'][f]), f


@pytest.mark.gpu
def test_path_count_is_zero_wherever_the_path_does_not_exist():
    """Mode 1 (the 4-multiplication tail) never takes it, whatever the switch says.  A complex trial whose spin blocks differ has
    no psi^H B on the handle -- such a trial's force bias does not contract the spin sum either, so its steps run two launches --
    and matches the oracle.  (A per-walker trial, psi_stride != 0, exists inside back-propagation windows only, and steps
    with a window configured never run the tail: the shape class excludes it.)"""
    M, N = SHAPES[1]
    for s in run(M, N, 6, 1, 1)['steps']:
        assert s['early'] == 0 and launches(s['trace'], 'prop_fused_kernel<false, 7, true, false>') == 1
    model, rng = build(M, K, N, N, True, seed=31)
    model.exp_order = 6
    phis = numpy.array([model.psi + 0.1 * (rng.rand(M, 2 * N) + 1j * rng.rand(M, 2 * N)) for _ in range(NW)])
    case = dict(model=model, phis=phis, w0=numpy.ones(NW), ot=numpy.array([ref.calc_overlap(p, model.psi, N, N) for p in phis]))
    walkers = [ref.new_walker(model, phis[i]) for i in range(NW)]
    want = oracle_steps(model, walkers, numpy.ones(NW, dtype=bool), 0, 2)
    dev = start(case, 2, 1)
    try:
        for step in range(2):
            s = one_step(dev, 'announced')
            assert s['early'] == 0 and launches(s['trace'], 'prop_fused_kernel<false, 7, true') == 0
            for i in range(NW):
                close(s['fields'][L.F_PHI][i], want[step]['phi'][i], TOL * (step + 1))
                close(s['fields'][L.F_WEIGHT][i], want[step]['weight'][i], TOL * (step + 1))
    finally:
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("M,N", SHAPES)
def test_second_propagator_rebuilds_psi_b(M, N):
    """Another time step's BH1 uploaded behind the first step: the next step, from the state read back from the device,
    matches the oracle of the new propagator, and still takes the path."""
    case, other = population(M, N, 6), population(M, N, 6, dt=0.005)
    m2 = other['model']
    assert not numpy.array_equal(case['model'].BH1, m2.BH1)
    dev = start(case, 2, 1)
    try:
        one_step(dev, 'announced')
        state = {f: dev.get(f) for f in (L.F_PHI, L.F_WEIGHT, L.F_OT, L.F_HYBRID_ENERGY)}
        dev.set_propagator(m2.BH1, m2.mf_shift, m2.dt, exp_order=6)
        walkers = []
        for i in range(NW):
            w = ref.new_walker(m2, state[L.F_PHI][i], weight=float(state[L.F_WEIGHT][i]))
            w['ot'] = w['ovlp'] = complex(state[L.F_OT][i])
            w['hybrid_energy'] = complex(state[L.F_HYBRID_ENERGY][i])
            walkers.append(w)
        want = oracle_steps(m2, walkers, case['w0'] != 0.0, 1, 1)[0]
        s = one_step(dev, 'announced')
        assert s['early'] == 2 * (NW - 2)
        for i in range(NW):
            if i == DEAD:
                continue
            for f, key in ((L.F_PHI, 'phi'), (L.F_WEIGHT, 'weight'), (L.F_OT, 'ot'), (L.F_HYBRID_ENERGY, 'ehyb'),
                           (L.F_XBAR, 'xbar')):
                close(s['fields'][f][i], want[key][i], TOL)
    finally:
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("on", [1, 0])
def test_a_step_launches_what_it_launched_before(on):
    """One propagator launch per step, the 3-multiplication tail kernel under its name of before; a Green's function launch only
    ahead of the first step, where nothing is cached; one weight_kernel on the split step and none elsewhere."""
    M, N = SHAPES[1]
    steps = run(M, N, 6, 2, on)['steps']
    assert [launches(s['trace'], 'prop_fused_kernel') for s in steps] == [1, 1, 1, 1]
    assert [launches(s['trace'], 'prop_fused_kernel<false, 7, true, true>') for s in steps] == [1, 1, 1, 1]
    assert [launches(s['trace'], 'greens_small_kernel') for s in steps] == [1, 0, 0, 0]
    assert [launches(s['trace'], 'weight_kernel') for s in steps] == [0, 0, 1, 0]
    assert launches(steps[1]['ghalf_trace'], 'greens_small_kernel') == 0


def test_switch_rejects_bad_values_and_null_handle():
    """No GPU: afq_set_step_tail_overlap takes 0 and 1 and nothing else, and refuses a null handle (a zeroed block stands in
    for the handle, which is only read after the value check)."""
    lib = L.load()
    assert lib.afq_set_step_tail_overlap(None, 0) == L.AFQ_EINVAL
    assert lib.afq_set_step_tail_overlap(None, 1) == L.AFQ_EINVAL
    block = ctypes.create_string_buffer(1 << 16)
    h = ctypes.cast(block, L._h)
    for bad in (-1, 2, 3, 1 << 20):
        assert lib.afq_set_step_tail_overlap(h, bad) == L.AFQ_EINVAL, bad
    assert block.raw == bytes(1 << 16)
