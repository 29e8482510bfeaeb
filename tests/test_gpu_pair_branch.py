"""Pair-branch population control on the device (afq_popcontrol_pair_branch, walkers/handler.py:225-251,340-412),
through the C ABI: the events and the trajectory the genuine reference produced (tests/golden/pair_branch.npz), random
populations against the host plan ``pair_branch_plan`` on both sides of the one-walker-per-thread boundary and of the
power-of-two padding of the sort, the state that travels with a clone, and ``Walkers.pop_control``.

Decisions (mult, slot origins, uniforms consumed, every copied field) are exact.  Weights are compared to a relative
1e-13: the device sums |w| chunk by chunk and numpy left to right, nw * 2^-53 at most apart, and three roundings follow
(the scale, the division, the pair sum); that is below 1e-13 up to the 1000 walkers used here.  Exact decisions need
every comparison clear of a rounding edge, which ``check_margins`` asserts on the host plan's inputs (1e-9 relative)."""
import ctypes

import numpy
import pytest

from pauxy_amd import _lib as L
from pauxy_amd import systems, trial as trial_mod
from pauxy_amd.comm import FakeComm
from pauxy_amd.context import release_context
from pauxy_amd.qmc.options import QMCOpts
from pauxy_amd.walkers.handler import Walkers, pair_branch_plan
from tests.helpers import generic_model, make_device

pytestmark = pytest.mark.gpu
WTOL = 1e-13
TRAJ_TOL = 1e-8           # the project's trajectory tolerance


def events(d):
    for k, name in enumerate(d['event_names']):
        yield str(name), {key[len('ev%d_' % k):]: d[key] for key in d if key.startswith('ev%d_' % k)}


def rel(a, b):
    a, b = numpy.asarray(a), numpy.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(numpy.max(numpy.abs(a - b) / numpy.maximum(numpy.abs(b), 1e-300))) if a.size else 0.0


@pytest.fixture(scope='module')
def model(golden):
    return generic_model(golden('pair_branch.npz'), 't_')


def walkers_on(model, nw, seed=1, nbp=0, steps=0):
    """nw distinct walkers; ``steps`` propagation steps make every scalar (and the field history) walker specific."""
    dev = make_device(model, nw)
    if nbp:
        dev.bp_configure(nbp)
    rng = numpy.random.RandomState(seed)
    nt = model.na + model.nb
    phi = model.psi[None] + 0.05 * (rng.rand(nw, model.M, nt) + 1j * rng.rand(nw, model.M, nt))
    dev.set(L.F_PHI, phi)
    dev.set(L.F_OT, dev.calc_overlap())
    for _ in range(steps):
        dev.propagate(rng.normal(size=(nw, dev.K)), 0.0)
    return dev


_HIP = []


def hip_runtime():
    """The HIP runtime the library is linked against, as a ctypes object of this file's own (prototypes set here do
    not touch the binding the package shares).  It has to be that runtime and no other copy in the process -- a
    buffer from a second runtime is not memory the handle's stream can copy into -- so the functions are looked up
    through the library itself: dlsym on a library's handle searches the library and then its dependencies."""
    if not _HIP:
        hip = ctypes.CDLL(L.LIB_PATH)
        hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        hip.hipFree.argtypes = [ctypes.c_void_p]
        _HIP.append(hip)
    return _HIP[0]


class DeviceBuffer(object):
    """Plain device memory to pack walkers into and unpack them from."""

    def __init__(self, dev, nbytes):
        self.hip, self.nbytes, self.ptr = hip_runtime(), nbytes, ctypes.c_void_p()
        dev.sync()                                   # (the handle's calls have made its device the current one)
        assert self.hip.hipMalloc(ctypes.byref(self.ptr), nbytes) == 0
        assert self.hip.hipMemset(self.ptr, 0, nbytes) == 0 and self.hip.hipDeviceSynchronize() == 0

    def download(self):
        out = numpy.empty(self.nbytes // 8)
        assert self.hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), self.ptr, self.nbytes, 2) == 0
        return out

    def upload(self, a):
        a = numpy.ascontiguousarray(a, dtype=numpy.float64)
        assert a.nbytes == self.nbytes
        assert self.hip.hipMemcpy(self.ptr, a.ctypes.data_as(ctypes.c_void_p), self.nbytes, 1) == 0

    def free(self):
        assert self.hip.hipFree(self.ptr) == 0


def snapshot(dev):
    """Every walker as afq_walker_pack lays it out, [nw, doubles]: phi, ot, hybrid energy, phase, eloc, unscaled weight,
    detR, weight, log detR [, phi_old, field history, phase and cosine factors, history length]."""
    per = dev.pack_bytes() // 8
    buf = DeviceBuffer(dev, 8 * per * dev.nw)
    for i in range(dev.nw):
        dev.pack(i, buf.ptr.value + 8 * per * i)
    dev.sync()
    out = buf.download().reshape(dev.nw, per)
    buf.free()
    return out


def restore(dev, snap):
    buf = DeviceBuffer(dev, snap.nbytes)
    buf.upload(snap)
    for i in range(dev.nw):
        dev.unpack(i, buf.ptr.value + 8 * snap.shape[1] * i)
    dev.sync()
    buf.free()


def columns(dev):
    """(unscaled weight, weight) columns of a snapshot."""
    n = 2 * dev.M * (dev.na + dev.nb)
    return n + 8, n + 10


def check_margins(w, min_weight, max_weight, u):
    """No comparison of the plan sits within 1e-9 (relative) of equality; exact ties between weights are allowed."""
    a = numpy.sort(numpy.abs(w), kind='mergesort')
    gaps = numpy.diff(a)
    assert numpy.all((gaps == 0) | (gaps > 1e-9 * a[1:])), 'two distinct weights within 1e-9'
    n = len(a)
    for p in range(n // 2):
        a_s, a_e = a[p], a[n - 1 - p]
        assert abs(a_s - min_weight) > 1e-9 * min_weight and abs(a_e - max_weight) > 1e-9 * max_weight, p
        if not (a_s < min_weight or a_e > max_weight):
            break
        q = a_e / (a_s + a_e)
        assert abs(u[p] - q) > 1e-9 * q, p


def run_event(dev, w_in, min_weight, max_weight, u, fetch=True):
    """One event against the host plan -> (snapshot before, snapshot after, plan)."""
    nw = dev.nw
    dev.set(L.F_WEIGHT, w_in)
    before = snapshot(dev)
    total_h = float(numpy.sum(numpy.abs(w_in)))
    w_s = w_in / (total_h / nw)
    check_margins(w_s, min_weight, max_weight, u)
    new_w, mult_h, pairs, nd_h = pair_branch_plan(w_s, min_weight, max_weight, u)
    mult, nd, total = dev.popcontrol_pair_branch(u, nw, min_weight, max_weight, fetch=fetch)
    after = snapshot(dev)
    if fetch:
        assert nd == nd_h and numpy.array_equal(mult, mult_h)
        assert abs(total - total_h) <= WTOL * total_h
    origin = numpy.arange(nw)
    for c, k in pairs:
        origin[k] = c
    ucol, wcol = columns(dev)
    rest = numpy.ones(before.shape[1], dtype=bool)
    rest[[ucol, wcol]] = False
    assert numpy.array_equal(after[:, rest].view(numpy.uint64), before[origin][:, rest].view(numpy.uint64))
    assert numpy.array_equal(after[:, ucol], w_in[origin])             # unscaled_weight travels with the walker
    err = rel(after[:, wcol], new_w)
    print('nw %d: %d pairs, weight error %.3e' % (nw, nd_h, err))
    assert err <= WTOL
    assert numpy.all(numpy.sign(after[:, wcol][mult_h == 1]) == numpy.sign(w_in[mult_h == 1]))
    assert abs(numpy.abs(after[:, wcol]).sum() - nw) <= 1e-12 * nw      # the total weight is conserved
    return before, after, (new_w, mult_h, pairs, nd_h, total_h)


def crowd(seed, n):
    """Light, ordinary and heavy walkers, every fifth negative, exact ties."""
    rng = numpy.random.RandomState(seed)
    if n <= 3:
        return numpy.array([0.05, 2.5, -1.3][:n]), rng.rand(n // 2)
    w = rng.choice([0.01, 0.05, 1.0, 1.0, 5.0, 8.0], n) * (0.5 + rng.rand(n))
    w[::5] *= -1.0
    if n > 4:
        w[3] = w[n - 1]
        w[n // 2] = -w[1]
    return w, rng.rand(n // 2)


def test_every_recorded_event(golden, model):
    d = golden('pair_branch.npz')
    for name, ev in events(d):
        nw = len(ev['w_in'])
        dev = walkers_on(model, nw, seed=nw, steps=1)
        u = numpy.full(nw // 2, 0.5)
        u[:ev['draws'].size] = ev['draws']
        before, after, plan = run_event(dev, ev['w_in'], float(ev['min_weight']), float(ev['max_weight']), u)
        ucol, wcol = columns(dev)
        assert plan[3] == ev['draws'].size, name
        assert rel(after[:, wcol], ev['w_out']) <= WTOL, name
        assert numpy.array_equal(after[:, ucol], ev['unscaled_out']), name
        assert numpy.array_equal(after[:, :wcol - 10], before[ev['origin']][:, :wcol - 10]), name       # phi: the slot origins
        dev.close()


@pytest.mark.parametrize('nw', [2, 3, 12, 255, 256, 257, 1000])
def test_random_populations_against_the_host_plan(model, nw):
    dev = walkers_on(model, nw, seed=nw, steps=1)
    w, u = crowd(100 + nw, nw)
    _, _, plan = run_event(dev, w, 0.1, 4.0, u)
    assert plan[3] >= 1 and (nw < 12 or plan[3] < nw // 2)              # pairs are acted on, and the loop ends early
    dev.close()


@pytest.mark.parametrize('nw', [4096, 8192])
def test_populations_above_the_default_lds_limit(model, nw):
    """4096 walkers are the first size whose sort needs more LDS than a launch gets by default, 8192 the largest the
    kernel serves (AFQ_PAIR_BRANCH_MAX_WALKERS); the fields are read back whole instead of walker by walker.  The
    same 1e-13 on the weights: the device adds at most 32 weights in sequence per thread and a dozen partial sums, numpy
    at most 128 in sequence and a few pairwise levels -- under 200 roundings of 2^-53 between the two totals, 2.2e-14."""
    dev = walkers_on(model, nw, seed=nw)
    w, u = crowd(100 + nw, nw)
    dev.set(L.F_WEIGHT, w)
    phi, ot = dev.get(L.F_PHI), dev.get(L.F_OT)
    total_h = float(numpy.sum(numpy.abs(w)))
    w_s = w / (total_h / nw)
    check_margins(w_s, 0.1, 4.0, u)
    new_w, mult_h, pairs, nd_h = pair_branch_plan(w_s, 0.1, 4.0, u)
    mult, nd, total = dev.popcontrol_pair_branch(u, nw, 0.1, 4.0)
    assert nd == nd_h and 1 <= nd < nw // 2 and numpy.array_equal(mult, mult_h)
    origin = numpy.arange(nw)
    origin[[k for _, k in pairs]] = [c for c, _ in pairs]
    assert numpy.array_equal(dev.get(L.F_PHI), phi[origin]) and numpy.array_equal(dev.get(L.F_OT), ot[origin])
    assert numpy.array_equal(dev.get(L.F_UNSCALED_WEIGHT), w[origin])
    err = rel(dev.get(L.F_WEIGHT), new_w)
    print('nw %d: %d pairs, weight error %.3e, total %.3e' % (nw, nd_h, err, abs(total - total_h) / total_h))
    assert err <= WTOL and abs(total - total_h) <= WTOL * total_h
    dev.close()


def test_more_walkers_than_the_kernel_serves_are_refused(model):
    dev = make_device(model, 8193)
    with pytest.raises(L.AfqError) as e:
        dev.popcontrol_pair_branch(numpy.full(4096, 0.5), 8193, 0.1, 4.0)
    assert e.value.code == -5                             # AFQ_EUNSUPPORTED
    dev.close()


def test_total_weight_feeds_the_weight_cap(model):
    dev = walkers_on(model, 12)
    w, u = crowd(7, 12)
    _, after, plan = run_event(dev, w, 0.1, 4.0, u)
    _, wcol = columns(dev)
    dev.cap_weights(0.04, -1.0)                      # 0.04 of the total the event measured (before scaling)
    cap = 0.04 * plan[4]
    got = dev.get(L.F_WEIGHT)
    want = numpy.where(numpy.abs(after[:, wcol]) > cap, cap, after[:, wcol])
    assert (numpy.abs(after[:, wcol]) > cap).any() and (numpy.abs(after[:, wcol]) < cap).any()
    assert rel(got, want) <= WTOL
    dev.close()


def test_event_without_read_back_gives_the_same_population(model):
    dev = walkers_on(model, 257, seed=3, steps=1)
    w, u = crowd(31, 257)
    before, after, _ = run_event(dev, w, 0.1, 4.0, u)
    restore(dev, before)
    assert dev.popcontrol_pair_branch(u, 257, 0.1, 4.0, fetch=False) == (None, None, None)
    assert numpy.array_equal(snapshot(dev).view(numpy.uint64), after.view(numpy.uint64))
    dev.close()


def test_back_propagation_state_arrives_with_the_clone(model):
    """nbp = 4: phi_old, the field history, the phase / cosine factors and the history length are columns of the snapshot
    that run_event compares slot by slot; here they are shown to differ between walkers, so the comparison means something."""
    dev = walkers_on(model, 12, seed=5, nbp=4, steps=3)
    w, u = crowd(7, 12)
    before, after, plan = run_event(dev, w, 0.1, 4.0, u)
    _, wcol = columns(dev)
    tail = before[:, wcol + 2:]
    assert tail.shape[1] == wcol - 10 + 2 * 4 * dev.K + 2 + 2
    hist = tail[:, wcol - 10:wcol - 10 + 2 * 4 * dev.K]
    assert len(set(hist[:, 0])) == 12 and numpy.count_nonzero(hist[0]) >= 3 * dev.K
    assert plan[3] >= 2
    for c, k in plan[2]:
        assert numpy.array_equal(after[k, wcol + 2:], tail[c]) and not numpy.array_equal(tail[k], tail[c])
    dev.close()


def test_kept_greens_function_travels_with_the_clone(model):
    """The step after an event uses the Green's function the step before it left (cloned with the walkers); it must give
    what a step from recomputed Green's functions gives.  Both are fp64 evaluations of the same matrices in another
    summation order: 1e-10 relative on the step's weights and overlaps, against O(1e-2) for a stale row."""
    w, u = crowd(7, 12)
    xi = numpy.random.RandomState(9).normal(size=(2, 12, model.hs_pot.shape[1]))
    res = []
    for recompute in (False, True):
        dev = walkers_on(model, 12, seed=5)
        dev.propagate(xi[0], 0.0)
        dev.set(L.F_WEIGHT, w)
        mult, nd, _ = dev.popcontrol_pair_branch(u, 12, 0.1, 4.0)
        assert nd >= 2
        if recompute:
            dev.set(L.F_PHI, dev.get(L.F_PHI))       # new walkers as far as the handle knows: nothing cached survives
        dev.propagate(xi[1], 0.0)
        res.append((dev.get(L.F_WEIGHT), dev.get(L.F_OT), dev.get(L.F_HYBRID_ENERGY)))
        dev.close()
    for a, b in zip(*res):
        assert rel(a, b) <= 1e-10


def test_collapsed_population_is_reported_and_nothing_changes(model):
    dev = walkers_on(model, 12, seed=2, steps=1)
    dev.set(L.F_WEIGHT, numpy.full(12, 1e-12))
    before = snapshot(dev)
    with pytest.raises(L.AfqError) as e:
        dev.popcontrol_pair_branch(numpy.full(6, 0.5), 12, 0.1, 4.0)
    assert e.value.code == L.AFQ_EWEIGHT
    assert numpy.array_equal(snapshot(dev).view(numpy.uint64), before.view(numpy.uint64))
    dev.close()


def test_too_few_uniforms_and_single_walker(model):
    dev = walkers_on(model, 12)
    u = numpy.full(6, 0.5)
    args = (0.1, 4.0, None, None, None)
    assert dev.lib.afq_popcontrol_pair_branch(dev.h, u.ctypes.data_as(ctypes.c_void_p), 5, 12.0, *args) == -1
    assert dev.lib.afq_popcontrol_pair_branch(dev.h, None, 6, 12.0, *args) == -1
    assert dev.lib.afq_popcontrol_pair_branch(dev.h, u.ctypes.data_as(ctypes.c_void_p), 6, 12.0, *args) == 0
    dev.close()
    one = walkers_on(model, 1)
    before = snapshot(one)
    assert one.lib.afq_popcontrol_pair_branch(one.h, None, 0, 1.0, *args) == 0
    assert numpy.array_equal(snapshot(one), before)
    one.close()


def test_trajectory_of_the_reference(golden, model):
    d = golden('pair_branch.npz')
    xi, every = d['t_xi'], int(d['t_every'])
    nsteps, nw = xi.shape[0], xi.shape[1]
    dev = make_device(model, nw)
    dev.set(L.F_PHI, d['t_phi0'])
    dev.set(L.F_OT, dev.calc_overlap())
    assert rel(dev.get(L.F_OT), d['t_ot0']) <= 1e-12
    used, event = 0, 0
    worst = 0.0
    for step in range(1, nsteps + 1):
        if step % every == 0:
            dev.reortho()
        dev.propagate(xi[step - 1], float(d['t_eshift']))
        if step % every == 0:
            n = int(d['t_ndraws'][event])
            u = numpy.full(nw // 2, 0.5)
            u[:n] = d['t_u'][used:used + n]
            mult, nd, _ = dev.popcontrol_pair_branch(u, nw, float(d['t_min_weight']), float(d['t_max_weight']))
            assert nd == n and (mult == 2).sum() == n, (step, nd, n)
            used, event = used + n, event + 1
        for field, key in ((L.F_WEIGHT, 't_weight'), (L.F_OT, 't_ot'), (L.F_HYBRID_ENERGY, 't_hybrid_energy'),
                           (L.F_UNSCALED_WEIGHT, 't_unscaled_weight')):
            want = d[key][step - 1]
            err = float(numpy.max(numpy.abs(dev.get(field) - want))) / max(1.0, float(numpy.max(numpy.abs(want))))
            worst = max(worst, err)
            assert err <= TRAJ_TOL, (step, key, err)
    print('trajectory: worst error %.3e' % worst)
    assert used == d['t_u'].size and (d['t_ndraws'] > 0).sum() >= 3
    dev.close()


@pytest.mark.parametrize('name', ['worked', 'odd11'])
def test_walkers_pop_control_leaves_the_host_stream_at_the_recorded_position(golden, name):
    d = golden('pair_branch.npz')
    ev = dict(events(d))[name]
    nw = len(ev['w_in'])
    na, nb = [int(x) for x in d['t_nelec']]
    s = systems.Generic((na, nb), numpy.array([d['t_h1e'], d['t_h1e']]), d['t_chol'], float(d['t_ecore']))
    t = trial_mod.SingleDetTrial(s, d['t_psi'])
    qmc = QMCOpts({'num_walkers': nw, 'timestep': 0.005}, s)
    qmc.ntot_walkers = qmc.nwalkers
    psi = Walkers(s, t, qmc, walker_opts={'population_control': 'pair_branch', 'min_weight': float(ev['min_weight']),
                                          'max_weight': float(ev['max_weight'])}, comm=FakeComm())
    for i, w in enumerate(psi.walkers):
        w.weight = float(ev['w_in'][i])
    numpy.random.seed(int(ev['seed']))
    psi.pop_control(FakeComm())
    assert numpy.random.rand() == float(ev['next_draw'])
    assert rel([w.weight for w in psi.walkers], ev['w_out']) <= WTOL
    assert numpy.array_equal([w.unscaled_weight for w in psi.walkers], ev['unscaled_out'])
    assert psi.total_weight == pytest.approx(float(ev['total_weight']), rel=WTOL)
    assert numpy.array_equal(numpy.bincount(ev['origin'], minlength=nw), psi.last_parent_ix)
    release_context(s, t)
