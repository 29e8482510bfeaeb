"""What a driver can do to a handle between two steps, as a table: configurations, warm states and one row per event.

The contract under test (tests/test_gpu_between_steps.py on the device, tests/test_between_steps_cpu.py over the numpy
stand-in): after ANY sequence of public calls the next steps and energies are those of a handle that never cached anything,
given the same model and walker state.  The library keeps a cached Green's function (FULL or SUM_ONLY, with the stamps of
its by-products), a closed-shell verdict, the Coulomb vectors of an energy evaluation, the step hand-over, psi^H B and the
per-determinant partials; every entry point that writes phi, moves a walker or changes the model has to drop or re-stamp the
right pieces, every reader has to put back what it took.  Nothing here needs a GPU: a row is a small function of a context
(device, model, configuration) that performs the event and returns the model the oracle has to use afterwards.

One case: start the configuration, reach the warm state, read the pure walker fields back (PHI, WEIGHT, UNSCALED_WEIGHT,
OT, HYBRID_ENERGY, PHASE, DETR, LOG_DETR -- never GHALF or G, which evaluate), run the event, read back again, build oracle
walkers from that state, then an announced step, an unannounced step, get(F_GHALF) and local_energy(), each against the
oracle.  Fields: on `tail` the device's own Philox draws restated on the host at the handle's counter; elsewhere an explicit
xi handed to both.

Configurations (the builders of the neighbouring files, no new shapes):
  rhf64   test_gpu_greens_cache.model_of: M = 24, K = 30, 5 + 5, 64 walkers       spin sum, closed verdict, vbias
  rhf24   the same with 24 walkers                                                no spin sum
  msd2    M = 12, 2 determinants, 3 + 3, 8 walkers                                per-determinant partials
  hub8x8  8 x 8 Hubbard, 46 + 46, 8 walkers                                       large path, diagonal sums
  tail    test_gpu_tail_overlap.population(97, 17, 6), 33 walkers, mode 2 scope 1 tail, early overlap, hand-over, psi^H B
  ueg     test_gpu_sizes.ueg_model_of(2.0, 2, 1, 1.0), 21 walkers                  the plane-wave fast step
Every population has one walker of weight zero since upload (slot DEAD); the closed-shell ones (rhf64, rhf24, tail) also
one open-shell walker (slot OPEN).

Every row of a configuration runs in all three warm states.  Rows left out of a configuration (Row.only / Row.never),
and why:
  set_phi_open, copy_open_closed, copy_closed_open, set_trial_real_closed, popcontrol_comb_local
                       closed-shell populations only (rhf64, rhf24, tail): elsewhere every walker is open-shell already, and
                       the two handles of the local comb are there for the Green's functions and the hand-over that travel
  set_trial_real_closed, set_trial_complex, set_system   not msd2: a multi-determinant handle refuses afq_set_trial; its row
                       is set_trial_multi, which sets the system up again as set_system does
  set_trial_multi, bp_update_msd, set_msd_force_bias, det_weights   msd2 only: they need a multi-determinant trial
  inverse_overlap, set_log_shift, estimates_rdm   not msd2: the library serves single-determinant trials only there
  bp_update, bp_update_ext, bp_update_pairing, itcf_update   not msd2 (its window is bp_update_msd), not hub8x8 (the device
                       back-propagates Hubbard systems with discrete fields only); itcf_update not ueg (the estimator is
                       the generic and Hubbard systems')
  set_exchange_algorithm_1 / _2   generic systems (rhf64, rhf24, tail, msd2): Hubbard and the electron gas have no Cholesky
                       exchange energy to choose an algorithm for
  local_energy_full_g  generic single-determinant systems; hubbard_energy_full_g: hub8x8; ueg_pair_sums, estimates_sf: ueg
  set_step_fusion_scope (0 and back to 1) tail only, set_step_fusion_scope_default (1 and back to 0) everywhere else: each
                       ends at the scope its configuration started with
  local_energy (warm state and last check) on ueg: afq_local_energy reads the full G as stored, which the plane-wave fast
                       step never builds -- estimates_update(True) + get(F_ENERGY) stands in, it evaluates what it needs
No row for afq_set_system_generic_c128 (EXEMPT): it is afq_set_system_generic with complex vectors and runs the same
set_dims, which frees the walkers and forgets trial and propagator, so the set_system row's re-setup holds for it.
"""
import copy
import ctypes
import functools

import numpy

from oracle import afqmc_ref as ref
from pauxy_amd import _lib as L

CONFIGS = ('rhf64', 'rhf24', 'msd2', 'hub8x8', 'tail', 'ueg')
WARM = ('full', 'sum', 'energy')
OPEN, DEAD = 1, 4
ESHIFT = 0.2
SEED = (2025, 5)                      # tests.test_gpu_step_fusion.SEED: what test_gpu_tail_overlap.start seeds the handle with
STATE = (L.F_PHI, L.F_WEIGHT, L.F_UNSCALED_WEIGHT, L.F_OT, L.F_HYBRID_ENERGY, L.F_PHASE, L.F_DETR, L.F_LOG_DETR)
CLOSED_CONFIGS = ('rhf64', 'rhf24', 'tail')


class Config(object):
    def __init__(self, name, model, nw, phis, w0, philox):
        self.name, self.model, self.nw, self.philox = name, model, nw, philox
        self.K = model.nfields
        self.phis, self.w0 = phis, w0
        self.ot = numpy.array([model.overlap(p) for p in phis])
        for a in (self.phis, self.w0, self.ot):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def configuration(name):
    if name == 'tail':
        from tests.test_gpu_tail_overlap import population, NW
        from tests import test_gpu_tail_overlap as tail
        assert (tail.OPEN, tail.DEAD) == (OPEN, DEAD) and (tail.ESHIFT, tail.SEED) == (ESHIFT, SEED)
        case = population(97, 17, 6)
        return Config(name, case['model'], NW, case['phis'], case['w0'], True)
    if name == 'ueg':
        from tests.test_gpu_sizes import ueg_model_of
        model, nw = ueg_model_of(2.0, 2, 1, 1.0), 21
        rng = numpy.random.RandomState(3)
        phis = numpy.array([model.psi + 0.05 * (rng.rand(model.M, 3) + 1j * rng.rand(model.M, 3)) for _ in range(nw)])
    else:
        from tests.test_gpu_greens_cache import model_of
        model, nw, phis = model_of(name)
        phis = numpy.array(phis)
    if name in CLOSED_CONFIGS:
        n = model.na
        rng = numpy.random.RandomState(23)
        phis[OPEN, :, n:] += 0.05 * (rng.rand(model.M, n) + 1j * rng.rand(model.M, n))
    w0 = numpy.ones(nw)
    w0[DEAD] = 0.0
    return Config(name, model, nw, phis, w0, False)


def upload_propagator(dev, model):
    kw = dict(hubbard_spin=model.kind == 'hubbard_spin') if model.kind in ('hubbard', 'hubbard_spin') else {}
    dev.set_propagator(model.BH1, model.mf_shift, model.dt, exp_order=model.exp_order, **kw)


def start(cfg, make, model=None):
    """A handle of the configuration with its population uploaded.  make(model, nw) -> device with walkers allocated
    (tests.helpers.make_device, or the stand-in's)."""
    dev = make(model or cfg.model, cfg.nw)
    if cfg.name == 'tail' and hasattr(dev, 'set_step_fusion'):
        dev.set_step_fusion(2)
        dev.set_step_fusion_scope(1)
        dev.set_step_tail_overlap(1)
        dev.set_step_handover(1)
    if cfg.philox:
        try:
            dev.rng_seed(*SEED)
        except NotImplementedError:
            pass
    dev.set(L.F_PHI, cfg.phis)
    dev.set(L.F_WEIGHT, cfg.w0)
    dev.set(L.F_OT, cfg.ot)
    return dev


def read_state(dev):
    return {f: dev.get(f) for f in STATE}


def upload_state(dev, state):
    for f in STATE:
        dev.set(f, state[f])


def same_bits(a, b):
    a, b = numpy.ascontiguousarray(a), numpy.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def is_live(weight):
    return numpy.abs(weight) > 1e-8           # qmc/afqmc.py:232


def is_closed(phi, na, nb):
    return na == nb and same_bits(phi[:, :na], phi[:, na:])


class Context(object):
    """What a row works on.  counter / seed follow the handle's Philox stream (tail); rng draws the explicit fields and
    whatever a row needs at random, the same for the device and the stand-in."""

    def __init__(self, cfg, make, warm):
        self.cfg, self.make, self.warm = cfg, make, warm
        self.model = cfg.model
        self.rng = numpy.random.RandomState(1234)
        self.seed, self.counter = SEED, 0
        self.dev = None
        self.others = []                      # further handles a row has opened
        self.window, self.warm_xi = 0, []     # steps of a configured window; the fields of the warm-up, for a second handle
        self.cache_off = False                # a device pointer was handed out: the handle keeps no Green's function any more

    @property
    def on_device(self):
        return hasattr(self.dev, 'estimates_fuse_next')

    def close(self):
        for d in self.others + [self.dev]:
            if d is not None:
                d.close()

    def fields(self):
        """-> (xi for the oracle, what to hand the device)"""
        cfg = self.cfg
        if cfg.philox and self.on_device:
            from tests.philox_ref import device_normals_fast
            xi = device_normals_fast(cfg.nw * cfg.K, self.seed[0], self.seed[1], self.counter).reshape(cfg.nw, cfg.K)
            self.counter += 1
            return xi, None
        xi = self.rng.normal(size=(cfg.nw, cfg.K))
        return xi, xi

    def step(self, announced, dev=None, xi=None):
        dev = dev or self.dev
        if xi is None:
            xi, given = self.fields()
        else:
            given = xi
        if announced and hasattr(dev, 'estimates_fuse_next'):
            dev.estimates_fuse_next()
        dev.propagate(given, ESHIFT)
        return xi

    def energy(self, dev=None):
        """local_energy() of the walkers' kept Green's function; on ueg the energy update that evaluates what it needs"""
        dev = dev or self.dev
        if not self.on_device:                 # (the stand-in caches nothing: whoever reads a Green's function evaluates it)
            dev.greens(want_G=False)
            return dev.local_energy()
        if self.cfg.name == 'ueg':
            dev.estimates_update(True)
            return dev.get(L.F_ENERGY)
        return dev.local_energy()

    def warm_up(self, dev=None):
        """full: the last step unannounced (kept == FULL); sum: announced (SUM_ONLY where the path has one); energy: full
        and an energy evaluation (vbias current).  tail: two steps, the second consumes a hand-over and leaves one."""
        first = dev is None
        for k in range(max(2 if self.cfg.name == 'tail' else 1, self.window)):
            xi = self.step(self.warm == 'sum', dev, None if first else self.warm_xi[k])
            if first:
                self.warm_xi.append(xi)
        if self.warm == 'energy':
            self.energy(dev)


def oracle_walkers(model, state):
    walkers = []
    for i in range(len(state[L.F_WEIGHT])):
        w = ref.new_walker(model, state[L.F_PHI][i], weight=float(state[L.F_WEIGHT][i]))
        w['ot'] = w['ovlp'] = complex(state[L.F_OT][i])
        w['unscaled_weight'] = float(state[L.F_UNSCALED_WEIGHT][i])
        w['hybrid_energy'] = complex(state[L.F_HYBRID_ENERGY][i])
        w['phase'] = complex(state[L.F_PHASE][i])
        w['detR'] = float(state[L.F_DETR][i])
        w['log_detR'] = float(state[L.F_LOG_DETR][i])
        walkers.append(w)
    return walkers


def clipped_force_bias(model, phi):
    _ovlp, ghalf, G = model.greens(phi)
    xbar = numpy.array(model.force_bias(ghalf, G), dtype=numpy.complex128)
    big = numpy.abs(xbar) > 1.0
    xbar[big] /= numpy.abs(xbar[big])
    return xbar


def oracle_step(model, walkers, xi):
    """One oracle step of every live walker -> what the device's fields are compared with."""
    live = [bool(is_live(w['weight'])) for w in walkers]
    xbar = [clipped_force_bias(model, w['phi']) if live[i] else None for i, w in enumerate(walkers)]
    for i, w in enumerate(walkers):
        if live[i]:
            ref.propagate_walker_phaseless(model, w, xi[i], ESHIFT)
    return dict(live=live, phi=[numpy.array(w['phi']) for w in walkers], weight=[w['weight'] for w in walkers],
                ot=[w['ot'] for w in walkers], ehyb=[w['hybrid_energy'] for w in walkers],
                phase=[w['phase'] for w in walkers], xbar=xbar)


def oracle_ghalf_energy(model, phi):
    """-> (per-spin Ghalf [na + nb, M] of the first determinant, (E, E1, E2)) of one walker"""
    psi = model.psi[0] if model.kind == 'generic_msd' else model.psi
    gh = numpy.concatenate(ref.greens_function(phi, psi, model.na, model.nb)[1], axis=0)
    _ovlp, ghalf, G = model.greens(phi)
    return gh, numpy.array(model.local_energy(G, ghalf), dtype=numpy.complex128)


# ---------------------------------------------------------------------------------------------------------- the rows
class Row(object):
    """name; kind: 'writer' | 'reader' | 'config'; fn(ctx) -> model after the event (None: unchanged); calls: the afq_*
    entry points the row is about; moves: which read-back fields the event must move by more than 1e-3 of their largest
    element on a live walker ('model': a model array instead; (): nothing -- the state must keep every bit);
    hands (tail): what counter [9] does on the step behind the event -- 'still' (the hand-over was dropped), 'on' (consumed
    by every walker live and closed on both sides of the event), 'off' (the path is gone for good), None (not looked at:
    a configured window keeps the tail from running); only / never: configurations; prepare(ctx): before the warm-up;
    oracle: the numpy stand-in has the methods."""

    def __init__(self, name, kind, fn, calls, moves=(), hands='kind', only=None, never=(), prepare=None, oracle=False):
        self.name, self.kind, self.fn, self.calls, self.moves = name, kind, fn, tuple(calls), moves
        self.hands = {'writer': 'still', 'config': 'still', 'reader': 'on'}[kind] if hands == 'kind' else hands
        self.only, self.never, self.prepare, self.oracle = only, tuple(never), prepare, oracle

    def runs_on(self, config):
        return (self.only is None or config in self.only) and config not in self.never


ROWS = []


def row(name, kind, calls, **kw):
    def deco(fn):
        ROWS.append(Row(name, kind, fn, calls, **kw))
        return fn
    return deco


def closed_live(ctx, state, n):
    """the first n slots past OPEN / DEAD that hold live walkers (closed-shell ones in a closed population)"""
    m = ctx.model
    out = [i for i in range(5, ctx.cfg.nw) if is_live(state[L.F_WEIGHT][i]) and
           (ctx.cfg.name not in CLOSED_CONFIGS or is_closed(state[L.F_PHI][i], m.na, m.nb))]
    assert len(out) >= n
    return out[:n]


def noise(ctx, shape, scale=0.05):
    return scale * (ctx.rng.rand(*shape) + 1j * ctx.rng.rand(*shape))


# -- walker writers
@row('set_phi_swap', 'writer', ['afq_walkers_set', 'afq_walkers_get'], moves=(L.F_PHI,), oracle=True)
def _(ctx):
    st = read_state(ctx.dev)
    a, b = closed_live(ctx, st, 2)
    phi, ot = st[L.F_PHI], st[L.F_OT]
    phi[[a, b]] = phi[[b, a]]
    ot[[a, b]] = ot[[b, a]]
    ctx.dev.set(L.F_PHI, phi)
    ctx.dev.set(L.F_OT, ot)


@row('set_phi_one', 'writer', ['afq_walkers_set'], moves=(L.F_PHI,), oracle=True)
def _(ctx):
    st = read_state(ctx.dev)
    k = closed_live(ctx, st, 3)[2]
    m = ctx.model
    phi = st[L.F_PHI][k]
    if ctx.cfg.name in CLOSED_CONFIGS:
        d = noise(ctx, (m.M, m.na))
        phi = phi + numpy.concatenate([d, d], axis=1)
    else:
        phi = phi + noise(ctx, phi.shape)
    ctx.dev.set(L.F_PHI, phi, first=k)
    ctx.dev.set(L.F_OT, numpy.array([m.overlap(phi)]), first=k)


@row('set_phi_open', 'writer', ['afq_walkers_set'], moves=(L.F_PHI,), only=CLOSED_CONFIGS, oracle=True)
def _(ctx):
    st = read_state(ctx.dev)
    k = closed_live(ctx, st, 2)[1]
    m = ctx.model
    phi = numpy.array(st[L.F_PHI][k])
    phi[:, m.na:] += noise(ctx, (m.M, m.nb))
    ctx.dev.set(L.F_PHI, phi, first=k)
    ctx.dev.set(L.F_OT, numpy.array([m.overlap(phi)]), first=k)


@row('set_ghalf_garbage', 'writer', ['afq_walkers_set'], moves=(), hands='on', oracle=True)
def _(ctx):
    m = ctx.model
    ctx.dev.set(L.F_GHALF, 3.0 + noise(ctx, (ctx.cfg.nw, m.na + m.nb, m.M), 1.0))


@row('set_ot_scaled', 'writer', ['afq_walkers_set'], moves=(L.F_OT,), hands='on', oracle=True)
def _(ctx):
    st = read_state(ctx.dev)
    ot = st[L.F_OT]
    ot[closed_live(ctx, st, 3)] *= 1.5
    ctx.dev.set(L.F_OT, ot)


@row('set_weight_revive_kill', 'writer', ['afq_walkers_set'], moves=(L.F_WEIGHT,), hands='on', oracle=True)
def _(ctx):
    st = read_state(ctx.dev)
    w = st[L.F_WEIGHT]
    assert w[DEAD] == 0.0
    w[DEAD] = 0.75                                        # dead since its upload: no kernel has ever evaluated anything for it
    w[closed_live(ctx, st, 1)[0]] = 0.0
    ctx.dev.set(L.F_WEIGHT, w)


@row('reset_weights', 'writer', ['afq_walkers_reset_weights'], moves=(L.F_WEIGHT,), hands='on', oracle=True)
def _(ctx):
    ctx.dev.reset_weights()                               # revives the dead walker too


@row('reortho', 'writer', ['afq_reortho'], moves=(L.F_PHI,), oracle=True)
def _(ctx):
    ctx.dev.reortho()


def copy_row(name, pick, moves=(L.F_PHI,)):
    @row(name, 'writer', ['afq_walkers_copy'], moves=moves, oracle=True,
         only=None if name in ('copy_closed_closed', 'copy_live_dead') else CLOSED_CONFIGS)
    def _(ctx):
        src, dst = pick(closed_live(ctx, read_state(ctx.dev), 2))
        ctx.dev.copy_walker(src, dst)


copy_row('copy_closed_closed', lambda c: (c[0], c[1]))
copy_row('copy_open_closed', lambda c: (OPEN, c[0]))
copy_row('copy_closed_open', lambda c: (c[0], OPEN))
copy_row('copy_live_dead', lambda c: (c[0], DEAD), moves=(L.F_PHI, L.F_WEIGHT))


@row('pack_unpack', 'writer', ['afq_walker_pack', 'afq_walker_unpack', 'afq_walker_pack_bytes'], moves=(L.F_PHI,))
def _(ctx):
    from tests.test_gpu_pair_branch import DeviceBuffer
    src = OPEN if ctx.cfg.name in CLOSED_CONFIGS else 2
    dst = closed_live(ctx, read_state(ctx.dev), 1)[0]
    buf = DeviceBuffer(ctx.dev, ctx.dev.pack_bytes())
    ctx.dev.pack(src, buf.ptr.value)
    ctx.dev.unpack(dst, buf.ptr.value)
    ctx.dev.sync()
    buf.free()


def comb_weights(nw):
    """a quarter of the walkers dead, a quarter of triple weight, the open-shell one among those: clones are forced"""
    w = numpy.ones(nw)
    w[1::4] = 3.0
    w[2::4] = 0.0
    assert w[OPEN] == 3.0
    return w


@row('popcontrol_comb', 'writer', ['afq_popcontrol_comb'], moves=(L.F_PHI,), oracle=True)
def _(ctx):
    ctx.dev.set(L.F_WEIGHT, comb_weights(ctx.cfg.nw))
    pix, _ = ctx.dev.popcontrol_comb(0.3, ctx.cfg.nw)     # (copies per slot)
    assert pix[OPEN] >= 2 and (numpy.asarray(pix) == 0).any()


@row('popcontrol_pair_branch', 'writer', ['afq_popcontrol_pair_branch'], moves=(L.F_PHI,))
def _(ctx):
    nw = ctx.cfg.nw
    w = numpy.ones(nw)
    w[OPEN], w[6] = 4.0, 0.05                             # above max_weight: cloned; below min_weight: killed or doubled
    ctx.dev.set(L.F_WEIGHT, w)
    u = numpy.full(nw // 2, 0.9)
    ctx.dev.popcontrol_pair_branch(u, float(nw), 0.5, 2.0)


@row('popcontrol_comb_local', 'writer', ['afq_popcontrol_comb_local', 'afq_comm_init_local'], moves=(L.F_PHI,),
     only=CLOSED_CONFIGS)
def _(ctx):
    from pauxy_amd.device import comm_init_local, popcontrol_comb_local
    nw = ctx.cfg.nw
    second = start(ctx.cfg, ctx.make)
    ctx.others.append(second)
    ctx.warm_up(second)                                    # the same steps: its kept Green's functions travel with its walkers
    comm_init_local([ctx.dev, second])
    w, heavy = numpy.ones(nw), numpy.ones(nw)              # a third of this handle's walkers light, of the other's heavy
    w[5::3], w[OPEN], heavy[0::3] = 0.1, 3.0, 2.1
    ctx.dev.set(L.F_WEIGHT, w)
    second.set(L.F_WEIGHT, heavy)
    pix, _ = popcontrol_comb_local([ctx.dev, second], 0.3, 2 * nw)
    mine = numpy.asarray(pix[:nw])                         # (copies per slot, this handle's first)
    assert mine[OPEN] >= 2 and (mine == 0).sum() > (mine - 1).clip(0).sum()     # more kills than clones: walkers come across


@row('apply_exponential', 'writer', ['afq_apply_exponential', 'afq_vhs', 'afq_vhs_count'], moves=(L.F_PHI,))
def _(ctx):
    xs = ctx.rng.normal(size=(ctx.cfg.nw, ctx.cfg.K)) + 0j
    ctx.dev.apply_exponential(10.0 * ctx.dev.vhs(xs))


@row('kinetic', 'writer', ['afq_kinetic'], moves=(L.F_PHI,))
def _(ctx):
    for _ in range(20):                                    # (one half-step of a small dt moves phi by dt: twenty of them)
        ctx.dev.kinetic()


# -- readers and borrowers: they must change nothing
def reader(name, calls, fn, **kw):
    ROWS.append(Row(name, 'reader', fn, calls, **kw))


def does(call):
    """a row that performs one call and leaves the model as it is"""
    def fn(ctx):
        call(ctx)
    return fn


def full_g(ctx, n=3):
    m = ctx.model
    return noise(ctx, (n, 2, m.M, m.M), 0.3)


reader('greens', ['afq_greens'], does(lambda ctx: ctx.dev.greens(want_G=False)), oracle=True)
reader('greens_full_G', ['afq_greens'], does(lambda ctx: ctx.dev.greens(want_G=True)), oracle=True)
reader('calc_overlap', ['afq_calc_overlap'], does(lambda ctx: ctx.dev.calc_overlap()), oracle=True)
reader('inverse_overlap', ['afq_inverse_overlap'], does(lambda ctx: ctx.dev.inverse_overlap()), never=('msd2',))


def _force_bias(ctx):
    ctx.dev.greens(want_G=ctx.cfg.name == 'ueg')
    ctx.dev.force_bias()


reader('force_bias', ['afq_force_bias'], _force_bias, oracle=True)


def _shift_fields(ctx):
    nw, K = ctx.cfg.nw, ctx.cfg.K
    ctx.dev.shift_fields(ctx.rng.normal(size=(nw, K)), noise(ctx, (nw, K)))


reader('shift_fields', ['afq_shift_fields'], _shift_fields)
reader('vhs', ['afq_vhs'], does(lambda ctx: ctx.dev.vhs(ctx.rng.normal(size=(ctx.cfg.nw, ctx.cfg.K)) + 0j)))
reader('local_energy', ['afq_local_energy'], does(lambda ctx: ctx.energy()), oracle=True)
reader('local_energy_full_g', ['afq_local_energy_full_g'], does(lambda ctx: ctx.dev.local_energy_full_g(full_g(ctx))),
       only=('rhf64', 'rhf24', 'tail'))
reader('correlations_full_g', ['afq_correlations_full_g'], does(lambda ctx: ctx.dev.correlations_full_g(full_g(ctx))))


def _pairing(ctx):
    M = ctx.model.M
    ctx.dev.set_pairing_bonds(numpy.array([numpy.roll(numpy.arange(M), 1), numpy.roll(numpy.arange(M), -1)]))
    ctx.dev.pairing_full_g(full_g(ctx, 2))
    ctx.dev.set_pairing_bonds(None)


reader('pairing_full_g', ['afq_pairing_full_g', 'afq_set_pairing_bonds'], _pairing)
reader('hubbard_energy_full_g', ['afq_hubbard_energy_full_g'],
       does(lambda ctx: ctx.dev.hubbard_energy_full_g(full_g(ctx))), only=('hub8x8',))
reader('ueg_pair_sums', ['afq_ueg_pair_sums'], does(lambda ctx: ctx.dev.ueg_pair_sums(full_g(ctx))), only=('ueg',))
reader('estimates_update', ['afq_estimates_update', 'afq_estimates_get'],
       does(lambda ctx: (ctx.dev.estimates_update(False), ctx.dev.estimates_get(zero=True))), oracle=True)
reader('estimates_update_energy', ['afq_estimates_update'], does(lambda ctx: ctx.dev.estimates_update(True)), oracle=True)


def _publish(ctx):
    ctx.dev.estimates_update_publish(True, zero=True)
    ctx.dev.estimates_get_end()


reader('estimates_update_publish', ['afq_estimates_update_publish', 'afq_estimates_get_end'], _publish)


def _get_begin_end(ctx):
    ctx.dev.estimates_get_begin(zero=False)
    ctx.dev.estimates_get_end()


reader('estimates_get_begin_end', ['afq_estimates_get_begin', 'afq_estimates_get_end'], _get_begin_end)


def _rdm(ctx):
    ctx.dev.estimates_rdm(True)
    ctx.dev.estimates_update(True)
    ctx.dev.estimates_rdm_get(zero=True)
    ctx.dev.estimates_rdm(False)


reader('estimates_rdm', ['afq_estimates_rdm', 'afq_estimates_rdm_get'], _rdm, never=('msd2',))


def _sf(ctx):
    ctx.dev.estimates_sf(True)
    ctx.dev.estimates_update(True)
    ctx.dev.estimates_sf_get(zero=True)
    ctx.dev.estimates_sf(False)


reader('estimates_sf', ['afq_estimates_sf', 'afq_estimates_sf_get'], _sf, only=('ueg',))
reader('get_ghalf', ['afq_walkers_get'], does(lambda ctx: ctx.dev.get(L.F_GHALF)), oracle=True)


def _get_G(ctx):
    ctx.dev.greens(want_G=True)                            # (G exists only once somebody asked for it)
    ctx.dev.get(L.F_G)


reader('get_G', ['afq_walkers_get'], _get_G, oracle=True)


def _window(ctx):
    ctx.window = 2
    ctx.dev.bp_configure(2)


def _bp_update(ctx):
    ctx.dev.bp_update(ctx.model.psi, 5, None)
    assert (ctx.dev.bp_steps() >= 0).all()


reader('bp_update', ['afq_bp_update', 'afq_bp_configure', 'afq_bp_steps'], _bp_update, prepare=_window, hands=None,
       never=('msd2', 'hub8x8'), oracle=True)


def _bp_update_ext(ctx):
    ctx.dev.bp_observables(two_rdm='correlation')
    ctx.dev.bp_ekt_chunks(0, 0)
    ctx.dev.bp_update(ctx.model.psi, 5, None, two_rdm=True)


reader('bp_update_ext', ['afq_bp_update_ext', 'afq_bp_observables', 'afq_bp_ekt_chunks'], _bp_update_ext, prepare=_window,
       hands=None, never=('msd2', 'hub8x8'))


def _bp_pairing(ctx):
    M = ctx.model.M
    ctx.dev.set_pairing_bonds(numpy.array([numpy.roll(numpy.arange(M), 1)]))
    ctx.dev.bp_observables(two_rdm='pairing')
    ctx.dev.bp_update(ctx.model.psi, 5, None, two_rdm=True)


reader('bp_update_pairing', ['afq_bp_pairing', 'afq_set_pairing_bonds'], _bp_pairing, prepare=_window, hands=None,
       never=('msd2', 'hub8x8'))


def _itcf_window(ctx):
    ctx.window = 2
    ctx.dev.itcf_configure(2)


reader('itcf_update', ['afq_itcf_update', 'afq_itcf_configure'], does(lambda ctx: ctx.dev.itcf_update(ctx.model.psi, 5)),
       prepare=_itcf_window, hands=None, never=('msd2', 'hub8x8', 'ueg'))
reader('bp_update_msd', ['afq_bp_update_msd'],
       does(lambda ctx: ctx.dev.bp_update_msd(ctx.model.psi, ctx.model.coeffs, 5, None)),
       prepare=_window, hands=None, only=('msd2',))
reader('det_weights', ['afq_walkers_det_weights'], does(lambda ctx: ctx.dev.det_weights()), only=('msd2',))
reader('log_ovlp_sums', ['afq_log_ovlp_sums'], does(lambda ctx: ctx.dev.log_ovlp_sums()))


# weights: they write the weight and nothing the caches are made of
@row('cap_weights', 'writer', ['afq_cap_weights'], moves=(L.F_WEIGHT,), hands='on', oracle=True)
def _(ctx):
    ctx.dev.cap_weights(0.5 / ctx.cfg.nw, float(ctx.cfg.nw))


@row('scale_weights', 'writer', ['afq_walkers_scale_weights'], moves=(L.F_WEIGHT,), hands='on', oracle=True)
def _(ctx):
    ctx.dev.scale_weights(1.7)


@row('set_weight_cap', 'config', ['afq_set_weight_cap'], moves=(), hands='on', oracle=True)
def _(ctx):
    ctx.dev.set_weight_cap(0.5)
    ctx.dev.set_weight_cap(0.0)


@row('rng_seed', 'reader', ['afq_rng_seed', 'afq_rng_normal', 'afq_rng_philox4x32'])
def _(ctx):
    ctx.seed, ctx.counter = (77, 3), 0
    ctx.dev.rng_seed(*ctx.seed)
    ctx.dev.rng_normal(16)                                 # (a draw for the host takes a counter value of the same stream)
    ctx.counter += 1
    ctx.dev.philox4x32(numpy.arange(6))


@row('traces_and_timers', 'reader', ['afq_enable_timers', 'afq_timers', 'afq_kernel_trace', 'afq_kernel_trace_stride',
                                     'afq_launch_trace', 'afq_launch_trace_get', 'afq_counters', 'afq_counters_ext',
                                     'afq_debug'])
def _(ctx):
    dev = ctx.dev
    dev.enable_timers(True)
    dev.kernel_trace(True)
    dev.kernel_trace_stride(0, 2)
    dev.launch_trace(True)
    dev.debug(sync_every_launch=True)
    dev.greens()                                           # ... something to time and trace
    dev.launch_trace_get()
    dev.timers(reset=True)
    dev.counters(reset=True, n=10)
    dev.debug(sync_every_launch=False)
    dev.launch_trace(False)
    dev.kernel_trace(False)
    dev.enable_timers(False)


# -- configuration
def with_(model, **kw):
    m = copy.copy(model)
    for k, v in kw.items():
        setattr(m, k, v)
    if 'dt' in kw:
        m.sqrt_dt = kw['dt'] ** 0.5
    return m


@row('set_propagator_dt', 'config', ['afq_set_propagator'], moves='model', oracle=True)
def _(ctx):
    m = ctx.model
    if ctx.cfg.name == 'tail':
        from tests.test_gpu_tail_overlap import population
        other = population(97, 17, 6, dt=0.005)['model']
    elif ctx.cfg.name in ('rhf64', 'rhf24'):
        from tests.test_gpu_sizes import build
        other = build(24, 30, 5, 5, False, dt=0.005)[0]
    else:                                                  # the same one-body factor for half the time step
        other = with_(m, dt=0.5 * m.dt)
    assert other.dt != m.dt and other.psi is not None
    upload_propagator(ctx.dev, other)
    return other


@row('set_propagator_same', 'config', ['afq_set_propagator'], moves=(), oracle=True)
def _(ctx):
    upload_propagator(ctx.dev, ctx.model)


@row('set_propagator_order', 'config', ['afq_set_propagator'], moves='model', oracle=True)
def _(ctx):
    other = with_(ctx.model, exp_order=3)
    upload_propagator(ctx.dev, other)
    return other


def orthonormal(a):
    return numpy.linalg.qr(a)[0]


@row('set_trial_real_closed', 'config', ['afq_set_trial'], moves='model', only=CLOSED_CONFIGS, oracle=True)
def _(ctx):
    m = ctx.model
    a = orthonormal(m.psi[:, :m.na].real + 0.1 * ctx.rng.rand(m.M, m.na)) + 0j
    other = with_(m, psi=numpy.concatenate([a, a], axis=1))
    ctx.dev.set_trial(other.psi)
    return other


@row('set_trial_complex', 'config', ['afq_set_trial'], moves='model', never=('msd2',), hands='off', oracle=True)
def _(ctx):
    m = ctx.model
    other = with_(m, psi=m.psi + noise(ctx, m.psi.shape))
    ctx.dev.set_trial(other.psi)
    return other


def set_up_again(ctx, model):
    """system, trial, propagator and walkers from scratch on the warm handle, and the read-back state uploaded"""
    dev, state = ctx.dev, read_state(ctx.dev)
    nw = ctx.cfg.nw
    if model.kind == 'generic':
        dev.set_system_generic(model.hs_pot, model.rchol, model.H1, model.ecore, model.na, model.nb)
    elif model.kind == 'hubbard':
        dev.set_system_hubbard(model.H1, model.U, model.na, model.nb)
    elif model.kind == 'ueg':
        dev.set_system_ueg(model.iA, model.iB, model.ikpq_i, model.ikpq_kpq, model.ipmq_i, model.ipmq_pmq, model.vqvec,
                           model.vol, model.H1diag, model.ecore, model.na, model.nb)
    if model.kind == 'generic_msd':
        from pauxy_amd import systems, trial as trial_mod
        s = systems.Generic((model.na, model.nb), model.H1.real, model.hs_pot, ecore=model.ecore)
        t = trial_mod.MultiDetTrial(s, (model.coeffs, model.psi))
        per = model.M * (model.na + model.nb)
        dev.set_system_generic(model.hs_pot, t._rchol[:per], model.H1, model.ecore, model.na, model.nb)
        dev.set_trial_multi(model.psi, model.coeffs, t._rchol)
    else:
        dev.set_trial(model.psi)
    upload_propagator(dev, model)
    dev.walkers_alloc(nw)
    upload_state(dev, state)


@row('set_system', 'config', ['afq_set_system_generic', 'afq_set_system_hubbard', 'afq_set_system_ueg', 'afq_set_trial',
                              'afq_walkers_alloc'], moves='model', never=('msd2',), oracle=True)
def _(ctx):
    m = ctx.model
    if m.kind == 'generic':                                # (the half-rotated vectors are linear in the Cholesky vectors)
        other = with_(m, hs_pot=0.8 * m.hs_pot, rchol=0.8 * m.rchol)
    elif m.kind == 'hubbard':
        other = with_(m, U=0.8 * m.U)
    else:
        other = with_(m, vqvec=0.8 * numpy.asarray(m.vqvec), H1diag=1.1 * numpy.asarray(m.H1diag))
    set_up_again(ctx, other)
    return other


@row('set_trial_multi', 'config', ['afq_set_trial_multi', 'afq_set_system_generic'], moves='model', only=('msd2',))
def _(ctx):
    m = ctx.model
    other = with_(m, coeffs=m.coeffs * numpy.array([1.0, 0.4 * numpy.exp(0.7j)]))
    set_up_again(ctx, other)
    return other


@row('walkers_alloc_same', 'config', ['afq_walkers_alloc'], moves=())
def _(ctx):
    state = read_state(ctx.dev)
    ctx.dev.walkers_alloc(ctx.cfg.nw)
    upload_state(ctx.dev, state)


@row('walkers_alloc_other', 'config', ['afq_walkers_alloc'], moves=())
def _(ctx):
    state = read_state(ctx.dev)
    ctx.dev.walkers_alloc(ctx.cfg.nw + 7)                  # (and back: the population of the configuration in new buffers)
    ctx.dev.walkers_alloc(ctx.cfg.nw)
    upload_state(ctx.dev, state)


def toggle(name, call, setter, away, back, **kw):
    def fn(ctx):
        getattr(ctx.dev, setter)(away)
        getattr(ctx.dev, setter)(back)
    ROWS.append(Row(name, 'config', fn, [call], **kw))


def _exchange(ctx):
    ctx.dev.set_exchange_algorithm(ctx.algorithm)
    assert ctx.dev.exchange_algorithm() == ctx.algorithm


def exchange(mode):
    def fn(ctx):
        ctx.algorithm = mode
        _exchange(ctx)
    ROWS.append(Row('set_exchange_algorithm_%d' % mode, 'config', fn, ['afq_set_exchange_algorithm', 'afq_exchange_algorithm'],
                    hands='on', only=('rhf64', 'rhf24', 'tail', 'msd2')))


exchange(1)
exchange(2)
toggle('set_propagator_closed_form', 'afq_set_propagator_closed_form', 'set_propagator_closed_form', 1, 0)
toggle('set_step_fusion', 'afq_set_step_fusion', 'set_step_fusion', 0, 2)
toggle('set_step_fusion_scope', 'afq_set_step_fusion_scope', 'set_step_fusion_scope', 0, 1, only=('tail',))
toggle('set_step_fusion_scope_default', 'afq_set_step_fusion_scope', 'set_step_fusion_scope', 1, 0, never=('tail',))
toggle('set_step_tail_overlap', 'afq_set_step_tail_overlap', 'set_step_tail_overlap', 0, 1)
toggle('set_step_handover', 'afq_set_step_handover', 'set_step_handover', 0, 1)


@row('set_msd_force_bias', 'config', ['afq_set_msd_force_bias', 'afq_msd_force_bias'], only=('msd2',))
def _(ctx):
    for mode in (1, 2):
        ctx.dev.set_msd_force_bias(mode)
        assert ctx.dev.msd_force_bias() == mode


@row('propagator_closed_form_get', 'reader', ['afq_propagator_closed_form'])
def _(ctx):
    ctx.dev.propagator_closed_form()


@row('set_log_shift', 'config', ['afq_set_log_shift'], hands='on', never=('msd2',), oracle=True)
def _(ctx):
    ctx.dev.set_log_shift(True, 0.3, 0.1)
    ctx.dev.set_log_shift(False)


def device_ptr(field):
    def fn(ctx):
        ptr, per = ctypes.c_void_p(), ctypes.c_int64()
        assert ctx.dev.lib.afq_walkers_device_ptr(ctx.dev.h, field, ctypes.byref(ptr), ctypes.byref(per)) == 0
        ctx.cache_off = True
    return fn


ROWS.append(Row('device_ptr_phi', 'config', device_ptr(L.F_PHI), ['afq_walkers_device_ptr'], hands='off'))
# (the cache is off for the life of the handle, and with it the tail that makes and takes the hand-over)
ROWS.append(Row('device_ptr_ghalf', 'config', device_ptr(L.F_GHALF), ['afq_walkers_device_ptr'], hands='off'))

ROW = {r.name: r for r in ROWS}
assert len(ROW) == len(ROWS)

# Entry points no row names, and why.
EXEMPT = {
    'afq_version': 'no handle', 'afq_create': 'life of the handle', 'afq_destroy': 'life of the handle',
    'afq_last_error': 'reads the error text', 'afq_sync': 'waits for the stream (the pack row calls it)',
    'afq_stream': 'hands out the stream, enqueues nothing',
    'afq_set_system_generic_c128': 'afq_set_system_generic with complex vectors: the same drop ahead of the same set_dims '
                                   '(tests/test_gpu_complex_chol.py holds its values)',
    'afq_propagate': 'the step itself, taken behind every row', 'afq_propagate_begin': 'the step itself: no row between the halves',
    'afq_propagate_finish': 'the step itself: no row between the halves',
    'afq_estimates_fuse_next': 'the announcement of the step behind every row',
    'afq_estimates_allreduce': 'needs peer processes', 'afq_estimates_allreduce_local': 'sums estimator blocks, no walker state',
    'afq_kernel_trace_get': 'pure getter of a trace', 'afq_kernel_issued_flops': 'pure getter of a counter',
    'afq_propagator_issued_flops': 'pure getter of a counter', 'afq_last_launch': 'pure getter of a trace',
    'afq_set_propagator_hirsch': 'Hirsch family: a propagator of its own', 'afq_hirsch_free_projection': 'Hirsch family',
    'afq_hirsch_single_site': 'Hirsch family', 'afq_propagate_hirsch_free': 'Hirsch family', 'afq_propagate_hirsch': 'Hirsch family',
    'afq_hirsch_kinetic': 'Hirsch family', 'afq_hirsch_two_body': 'Hirsch family', 'afq_hirsch_finish': 'Hirsch family',
    'afq_comm_unique_id': 'needs peer processes', 'afq_comm_available': 'no handle', 'afq_comm_init': 'needs peer processes',
    'afq_comm_init_ipc': 'needs peer processes', 'afq_comm_destroy': 'needs peer processes',
    'afq_comm_set_transport': 'needs peer processes', 'afq_comm_set_capacity': 'needs peer processes',
    'afq_comm_set_timeout': 'needs peer processes', 'afq_comm_probe': 'needs peer processes',
    'afq_comm_stats': 'pure getter of counters', 'afq_comm_parent_ix': 'needs peer processes',
    'afq_debug_guard_check': 'reads the guard bands, touches no walker state',
    'afq_debug_guard_report': 'reads the log of guard-band violations, touches no walker state',
    'afq_debug_guard_reset': 'clears the log of guard-band violations, touches no walker state',
}


def cases(configs=CONFIGS, warms=WARM):
    """(config, warm state, row name) of the device suite: every row of a configuration in every warm state."""
    return [(c, w, r.name) for c in configs for w in warms for r in ROWS if r.runs_on(c)]


# ---------------------------------------------------------------------------------------------------- running a case
def moved(before, after, live):
    """largest change of a live walker's entry of each field, relative to the field's largest element"""
    out = {}
    for f in STATE:
        a, b = numpy.asarray(after[f]), numpy.asarray(before[f])
        scale = max(float(numpy.abs(b).max()), float(numpy.abs(a).max()), 1e-300)
        d = numpy.abs(a - b).reshape(len(a), -1).max(axis=1)
        out[f] = float(d[live].max()) / scale if live.any() else 0.0
    return out


def model_moved(a, b):
    for key in ('BH1', 'psi', 'hs_pot', 'coeffs', 'mf_shift', 'vqvec'):
        x, y = getattr(a, key, None), getattr(b, key, None)
        if x is not None and y is not None and not isinstance(x, (list, tuple)):
            x, y = numpy.asarray(x), numpy.asarray(y)
            if x.shape == y.shape and numpy.abs(x - y).max() > 1e-3 * numpy.abs(x).max():
                return True
    return any(abs(getattr(a, k) - getattr(b, k)) > 1e-3 * abs(getattr(a, k)) for k in ('dt', 'exp_order', 'U') if hasattr(a, k))


REBUILT = ('set_system', 'set_trial_multi', 'walkers_alloc_same', 'walkers_alloc_other')


def check_teeth(r, out):
    """A writer or configuration row moved what it claims, by more than 1e-3 of the field's largest element on a live walker
    (a condition on the inputs: a stale operand of that size cannot hide under the tolerance of a step that is linear in phi
    through well-conditioned factors); a row that claims no walker field left every bit of the read-back state."""
    before, after = out['before'], out['after']
    live = is_live(before[L.F_WEIGHT]) | is_live(after[L.F_WEIGHT])
    if r.moves == 'model':
        assert model_moved(out['ctx'].cfg.model, out['model']), r.name
    elif r.moves:
        by = moved(before, after, live)
        assert all(by[f] > 1e-3 for f in r.moves), (r.name, by)
    if r.moves == () or r.moves == 'model':
        for f in STATE:
            assert same_bits(before[f], after[f]), (r.name, f)


def run_case(config, warm, name, make):
    """-> dict(before, after, model, steps=[(device fields, oracle)], ghalf, energy, want_ghalf, want_energy, handed)
    The assertions are the callers'; this only drives the handle and the oracle through the same case."""
    cfg, r = configuration(config), ROW[name]
    ctx = Context(cfg, make, warm)
    try:
        ctx.dev = dev = start(cfg, make)
        if r.prepare:
            r.prepare(ctx)
        counted = lambda: int(dev.counters(n=10)[9]) if ctx.on_device and config == 'tail' else 0
        ctx.warm_up()
        before, warm_handed = read_state(dev), counted()
        model = r.fn(ctx)
        if model is None:
            model = ctx.model
        after = read_state(dev)
        handed = [counted()]                  # (behind the event: a row may have reset the counters)
        walkers = oracle_walkers(model, after)
        out = dict(before=before, after=after, model=model, steps=[], handed=handed, warm_handed=warm_handed, ctx=ctx)
        fields = (L.F_PHI, L.F_WEIGHT, L.F_OT, L.F_HYBRID_ENERGY, L.F_PHASE) + ((L.F_XBAR,) if ctx.on_device else ())
        for announced in (True, False):
            xi = ctx.step(announced)
            got = {f: dev.get(f) for f in fields}
            handed.append(counted())
            out['steps'].append((got, oracle_step(model, walkers, xi)))
        if ctx.cache_off or not ctx.on_device:    # (as on a handle that never cached: whoever reads Ghalf evaluates it first)
            dev.greens(want_G=False)
        out['ghalf'] = dev.get(L.F_GHALF)
        out['energy'] = ctx.energy()
        want = [oracle_ghalf_energy(model, w['phi']) for w in walkers]
        out['want_ghalf'], out['want_energy'] = [g for g, _ in want], [e for _, e in want]
        return out
    finally:
        ctx.close()
