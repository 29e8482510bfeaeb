"""Walker populations that reach the decision branches of the phaseless constraint, with the oracle's verdict per walker.

The branches (propagation/continuous.py:140-158, 202-230, 264-318): the force-bias bound |xbar_n| > 1 -> xbar_n / |xbar_n|,
the hybrid / local-energy bound eshift +- sqrt(2 / dt) (none for |eshift| < 1e-10), the phase kill cos(dtheta) <= 0 ->
weight 0, an infinite importance function -> weight 0, and a vanishing one -> back-propagation factor 0.

``build(name)`` returns ``(model, phis, weights, xi, eshift, extra)`` of a named case; ``oracle_step`` advances a population
by one step with ``oracle/afqmc_ref.py`` and returns what the reference decided for every walker; ``check_case`` asserts, on
the reference alone, that no decision of the case is marginal and that each branch is reached by the share of walkers the
case is meant to have.  Everything here runs on the CPU: a seed that misses a branch fails in
tests/test_constraint_cases_cpu.py as a fixture error, never as a device mismatch.

How the branches are reached.  The force bias vanishes for a walker that equals the trial and grows with the distance from
it, so the walkers are psi + a_w * noise with amplitudes a_w graded from 0: near walkers keep all their fields, far ones
have theirs clipped.  The synthetic Cholesky vectors are tiny (force bias ~ 0.05 at any distance), so every second one is
scaled up before the model's derived arrays are built; lattice and plane-wave models take a larger U dt / dt instead (the
plane-wave force bias goes as sqrt(dt / rs) and the kinetic exponent as dt / rs^2, hence rs = 1 with a very long step).
The unbounded energies then spread over many widths 2 sqrt(2 / dt) of the bound; a third of the live walkers get fields
scaled DOWN to 0.05, which leaves their hybrid energies within a few units of each other, and the energy shift of a case
sits among those: they are the walkers inside the bound.  The phase of the overlap ratio grows with the fields: another
third gets fields scaled up.  The cases are two-step fixtures, not physics: time steps and couplings are whatever reaches
the branches with well-conditioned overlaps.
"""
import cmath
import functools
import math

import numpy

from oracle import afqmc_ref as ref
from pauxy_amd import systems, trial as trial_mod
from pauxy_amd.propagation import setup
from tests.philox_ref import device_normals_fast

GUARD = 1e-6            # no decision of a case is closer to its threshold than this (the device agrees to ~1e-12)
# What one rounding error in a walker may do to the reference's own result of a step, in the measure of the device tests'
# ``close``: a hundredth of their 1e-9.  A case beyond this compares rounding histories, not code (a plane-wave case with
# rs = 1, dt = 16 moved by 4e-8: the trial's rows of exp(V) phi are small differences of large Taylor terms there).
CONDITIONING = 1e-11


# ---------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------
def generic_model(M, K, na, nb, dt, closed=False, seed=3, chol_scale=1.0):
    """Synthetic generic Hamiltonian whose Cholesky vectors are scaled BEFORE everything derived from them (h1e_mod, the
    half-rotated vectors, the mean-field shift, BH1) is built.  closed: the real RHF-type trial (one block for both
    spins); otherwise a complex trial with distinct spin blocks."""
    s0 = systems.synthetic_generic(M, K, (na, nb), seed=seed)
    s = systems.Generic((na, nb), s0.H1, s0.hs_pot * numpy.asarray(chol_scale, dtype=float), ecore=0.37)
    if closed:
        assert na == nb
        t = trial_mod.rhf_trial_generic(s)
    else:
        rng = numpy.random.RandomState(seed + 50)
        psi = numpy.array(trial_mod.rhf_trial_generic(s).psi)
        t = trial_mod.SingleDetTrial(s, psi + 0.05 * (rng.rand(M, na + nb) + 1j * rng.rand(M, na + nb)))
    BH1, mf = setup.generic_propagator_arrays(s, t, dt)
    return ref.RefModel('generic', M, na, nb, numpy.array(t.psi), BH1, mf, dt, hs_pot=s.hs_pot, rchol=t._rchol,
                        H1=s.H1.astype(complex), ecore=s.ecore)


def msd_model(M, K, na, nb, ndet, dt, seed=7, chol_scale=1.0):
    s0 = systems.synthetic_generic(M, K, (na, nb), seed=seed)
    s = systems.Generic((na, nb), s0.H1, s0.hs_pot * numpy.asarray(chol_scale, dtype=float), ecore=0.37)
    t0 = trial_mod.rhf_trial_generic(s)
    rng = numpy.random.RandomState(seed + 50)
    nt = na + nb
    dets = numpy.array([t0.psi + (0.0 if d == 0 else 0.05) * (rng.rand(M, nt) + 1j * rng.rand(M, nt))
                        for d in range(ndet)])
    coeffs = (rng.rand(ndet) + 0.2) * numpy.exp(1j * rng.rand(ndet))
    t = trial_mod.MultiDetTrial(s, (coeffs, dets), init=t0.psi)
    BH1, mf = setup.generic_propagator_arrays(s, t, dt)
    model = ref.RefModel('generic_msd', M, na, nb, dets, BH1, mf, dt, coeffs=coeffs, hs_pot=s.hs_pot,
                         H1=s.H1.astype(complex), ecore=s.ecore)
    model.centre = numpy.array(t0.psi)
    return model


def ueg_model(rs, na, nb, ecut, dt):
    s = systems.UEG(rs, na, nb, ecut)
    t = trial_mod.hartree_fock_ueg(s)
    BH1, mf = setup.ueg_propagator_arrays(s, t, dt)
    H1diag = numpy.array([numpy.diag(s.H1[0]), numpy.diag(s.H1[1])])
    return ref.RefModel('ueg', s.nbasis, na, nb, numpy.array(t.psi), BH1, mf, dt, iA=s.iA, iB=s.iB, H1diag=H1diag,
                        vqvec=s.vqvec, vol=s.vol, ikpq_i=s.ikpq_i, ikpq_kpq=s.ikpq_kpq, ipmq_i=s.ipmq_i,
                        ipmq_pmq=s.ipmq_pmq, ecore=s.ecore)


def hubbard_model(nx, ny, na, nb, U, spin, dt):
    s = systems.Hubbard(nx, ny, na, nb, U)
    t = trial_mod.uhf_trial_hubbard(s, ueff=0.4)
    BH1, mf = setup.hubbard_propagator_arrays(s, t, dt, not spin)
    return ref.RefModel('hubbard_spin' if spin else 'hubbard', nx * ny, na, nb, numpy.array(t.psi), BH1, mf, dt, U=U,
                        H1=s.T.astype(complex))


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's verdict
# ---------------------------------------------------------------------------------------------------------------------
def new_walkers(model, phis, weights, hybrid_energy=None):
    walkers = []
    for i, (p, w0) in enumerate(zip(phis, weights)):
        w = ref.new_walker(model, p, float(w0))
        if hybrid_energy is not None:
            w['hybrid_energy'] = complex(hybrid_energy[i])
        walkers.append(w)
    return walkers


def oracle_step(model, walkers, xi, eshift, hybrid=True, cap=None):
    """One step of every walker by the oracle (qmc/afqmc.py:231-236: walkers with |weight| <= 1e-8 are not propagated, the
    cap ``(frac, total_weight)`` is applied to all of them).  Returns one dict per walker: ``live``; for a live walker the
    unclipped force bias ``xbar_raw`` [K], the clipped-field ``mask`` [K], the clipped ``xbar`` and the shifted fields
    ``xshifted``, the counts ``nfb`` / ``nhe`` the oracle returned, the unbounded energy ``e_unbounded`` the bound looked
    at (hybrid energy, or the local energy when not hybrid), the ``side`` of the bound it was on (-1 below, 0 inside or no
    bound, +1 above), ``cos`` = cos(dtheta) before the clamp at 0, the three distances from the
    thresholds and the distance of arg(ratio) from the branch cut of the logarithm; for every walker the state after the
    step: weight, ot, hybrid_energy, eloc, phase, phi."""
    dt = model.dt
    ebound = math.sqrt(2.0 / dt)
    es = complex(eshift).real
    out = []
    for i, w in enumerate(walkers):
        v = dict(live=abs(w['weight']) > 1e-8)
        if v['live']:
            x = numpy.asarray(xi[i], dtype=float)
            ovlp, Ghalf, G = model.greens(w['phi'])
            raw = numpy.array(model.force_bias(Ghalf, G), dtype=complex)
            xs, cmf, cfb, _ = ref.shift_fields(x, raw, model.mf_shift, model.sqrt_dt)
            v['nfb'], v['nhe'] = ref.propagate_walker_phaseless(model, w, x, eshift, hybrid)
            ratio = w['ot'] / ovlp
            if hybrid:
                e = -(cmath.log(ratio) + cfb + cmf) / dt
                efin = complex(w['hybrid_energy'])
                dtheta = (-dt * efin - cfb).imag
            else:
                e = complex(w['eloc'])
                dtheta = cmath.phase(ratio)
            bounded = abs(eshift) >= 1e-10
            v['side'] = 0 if not bounded else (1 if e.real > es + ebound else (-1 if e.real < es - ebound else 0))
            v.update(xbar_raw=raw, mask=numpy.abs(raw) > 1.0, xbar=x - xs, xshifted=xs, e_unbounded=e,
                     cos=math.cos(dtheta),
                     margin_fb=float(numpy.min(numpy.abs(numpy.abs(raw) - 1.0))),
                     margin_e=min(abs(e.real - (es + ebound)), abs(e.real - (es - ebound))) if bounded else numpy.inf,
                     margin_cos=abs(math.cos(dtheta)), margin_arg=math.pi - abs(cmath.phase(ratio)))
        if cap is not None and abs(w['weight']) > cap[0] * cap[1]:
            w['weight'] = cap[0] * cap[1]
        v.update(weight=float(w['weight']), ot=complex(w['ot']), hybrid_energy=complex(w['hybrid_energy']),
                 eloc=complex(w['eloc']), phase=complex(w['phase']), phi=w['phi'].copy())
        out.append(v)
    return out


def summary(verdicts):
    """Branch counts of one step: what tests/test_constraint_cases_cpu.py prints and check_case looks at."""
    live = [v for v in verdicts if v['live']]
    pairs = sum(v['mask'].size for v in live)
    return dict(nw=len(verdicts), live=len(live), pairs=pairs, clipped=int(sum(v['mask'].sum() for v in live)),
                walkers_unclipped=sum(1 for v in live if not v['mask'].any()),
                walkers_mixed=sum(1 for v in live if v['mask'].any() and not v['mask'].all()),
                nfb=int(sum(v['nfb'] for v in live)), nhe=int(sum(v['nhe'] for v in live)),
                above=sum(1 for v in live if v['side'] > 0), below=sum(1 for v in live if v['side'] < 0),
                inside=sum(1 for v in live if v['side'] == 0),
                killed=sum(1 for v in live if v['weight'] == 0.0), survived=sum(1 for v in live if v['weight'] != 0.0),
                margin_fb=min(v['margin_fb'] for v in live), margin_e=min(v['margin_e'] for v in live),
                margin_cos=min(v['margin_cos'] for v in live), margin_arg=min(v['margin_arg'] for v in live))


# ---------------------------------------------------------------------------------------------------------------------
# populations
# ---------------------------------------------------------------------------------------------------------------------
def population(model, nw, amax, xi_big, seed, closed=False, philox=None, mixed=False):
    """nw walkers psi + a_w * noise (complex normal, the same for both spins when ``closed``) with a_w graded from 0 to
    amax over the live walkers; every fifth walker starts dead (weight 0) and one more sits at 5e-9, below the 1e-8 the
    driver propagates.  Fields of two steps: standard normals, scaled by 0.05 / 1 / ``xi_big`` in turn over the live
    walkers; with ``philox`` = (seed, stream) the numbers the device draws itself at counters 0 and 1 (no scaling then).
    ``mixed``: every third walker from index 1 is opened -- 0.05 * complex normal noise on its beta block, from a stream
    of its own behind every other draw, so that no other case sees it."""
    rng = numpy.random.RandomState(seed)
    M, na, nt, K = model.M, model.na, model.na + model.nb, model.nfields
    centre = getattr(model, 'centre', model.psi)
    weights = 0.5 + rng.rand(nw)
    weights[2::5] = 0.0
    if nw >= 6:
        weights[5] = 5e-9
    live = numpy.nonzero(numpy.abs(weights) > 1e-8)[0]
    amps = numpy.zeros(nw)
    amps[live] = amax * numpy.linspace(0.0, 1.0, len(live)) ** 2            # (more walkers near the trial than far)
    amps[weights <= 1e-8] = 0.5 * amax
    scale = numpy.ones(nw)
    scale[live[0::3]] = 0.05
    scale[live[2::3]] = xi_big
    phis = numpy.empty((nw, M, nt), dtype=complex)
    for i in range(nw):
        if closed:
            n = rng.normal(size=(M, na)) + 1j * rng.normal(size=(M, na))
            n = numpy.concatenate([n, n], axis=1)
        else:
            n = rng.normal(size=(M, nt)) + 1j * rng.normal(size=(M, nt))
        phis[i] = centre + amps[i] * n
    if philox is None:
        xi = [rng.normal(size=(nw, K)) * scale[:, None] for _ in range(2)]
    else:
        xi = [device_normals_fast(nw * K, philox[0], philox[1], c).reshape(nw, K) for c in range(2)]
    ehyb0 = rng.normal(size=nw) + 0.1j * rng.normal(size=nw)
    if mixed:
        own = numpy.random.RandomState(seed + 1000)
        for i in range(1, nw, 3):
            phis[i, :, na:] += 0.05 * (own.normal(size=(M, nt - na)) + 1j * own.normal(size=(M, nt - na)))
    return phis, weights, xi, ehyb0


GEN = dict(kind='generic', dt=0.05, top=300.0, amax=0.5, xi_big=2.0)
# name -> what builds the case.  model arguments; nw; eshift; ``kernels``: substrings of launch names that must show up
# in the step's launch trace, ``absent``: ones that must not; ``checks``: the coverage conditions check_case asserts.
ALL = ('fb', 'ebound', 'kill')
CASES = {}


def _case(name, **kw):
    spec = dict(seed=11, closed=False, hybrid=True, philox=None, cap=None, overflow=False, bp=None, checks=ALL,
                kernels=(), absent=(), msd_fb_mode=0, eshift=0.0,
                closed_deal=False, mixed=False)
    spec.update(kw)
    CASES[name] = spec


def names():
    return sorted(CASES)


_models = {}


def _model(spec):
    key = repr(sorted((k, repr(v)) for k, v in spec['model'].items()))
    if key not in _models:
        a = dict(spec['model'])
        kind = a.pop('kind')
        if kind in ('generic', 'msd'):
            top = a.pop('top')
            # every second Cholesky vector scaled up: those are the fields whose force bias passes 1 away from the trial
            a['chol_scale'] = numpy.where(numpy.arange(a['K']) % 2 == 0, top, 1.0) if top else 1.0
        _models[key] = dict(generic=generic_model, msd=msd_model, ueg=ueg_model, hubbard=hubbard_model)[kind](**a)
    return _models[key]


def build(name):
    """-> (model, phis, weights, xi, eshift, extra).  xi: the fields of the first step; extra: ``xi2`` (second step),
    ``ehyb0`` (F_HYBRID_ENERGY / F_ELOC before the first step), and the case's settings (hybrid, philox, cap, bp,
    kernels, absent, checks, msd_fb_mode, closed)."""
    spec = CASES[name]
    model = _model(spec)
    phis, weights, xi, ehyb0 = population(model, spec['nw'], spec['amax'], spec['xi_big'], spec['seed'],
                                          spec['closed'], spec['philox'], spec['mixed'])
    ehyb0 = ehyb0 + spec['eshift']
    if spec['overflow']:
        # exp(-dt (0.5 (e + e_old) - eshift)): e_old = -1e6 -> inf (weight 0 by the isinf branch), +1e6 -> 0 (weight 0,
        # and a back-propagation factor that must be 0, not 0 / 0)
        live = numpy.nonzero(numpy.abs(weights) > 1e-8)[0]
        ehyb0[live[1::4]] = -1e6
        ehyb0[live[3::4]] = 1e6
    extra = dict(spec, xi2=xi[1], ehyb0=ehyb0)
    return model, phis, weights, xi[0], spec['eshift'], extra


@functools.lru_cache(maxsize=None)
def run_oracle(name):
    """The case through two steps of the oracle, computed once per session and shared: -> dict(case, ot0, verdicts
    [step 1, step 2], estimates, bp_steps, bp_est).  ``estimates``: estimators/mixed.py:180-225 with the energy, over
    the walkers as the second step leaves them.  With back-propagation configured (``bp`` = window length = 2):
    ``bp_steps`` per walker and ``bp_est`` = [3 energies, denominator, G.flatten()] of the window the second step closes,
    weights restored partially (the cosine factor of a killed walker is 0: the full restoration divides by it).
    Nobody may change what this returns."""
    case = build(name)
    model, phis, weights, xi, eshift, extra = case
    walkers = new_walkers(model, phis, weights, extra['ehyb0'])
    ot0 = numpy.array([w['ot'] for w in walkers])
    for w, e in zip(walkers, extra['ehyb0']):
        w['eloc'] = complex(e)
    if extra['bp']:
        for w in walkers:
            w['bp'] = ref.bp_new(model.nfields, extra['bp'])
            w['phi_old'] = w['phi'].copy()
    verdicts = [oracle_step(model, walkers, x, eshift, extra['hybrid'], extra['cap']) for x in (xi, extra['xi2'])]
    est = numpy.zeros(10, dtype=numpy.complex128)
    ref.mixed_update(model, est, walkers, 0, 1)
    out = dict(case=case, ot0=ot0, verdicts=verdicts, estimates=est, bp_steps=None, bp_est=None)
    if extra['bp']:
        out['bp_steps'] = numpy.array([w['bp']['step'] for w in walkers])
        out['bp_est'] = numpy.zeros(4 + 2 * model.M * model.M, dtype=numpy.complex128)
        ref.bp_update(model, walkers, 10, out['bp_est'], 'partial')
    return out


def sensitivity(name, draws=2):
    """The first step of a case once more with every element of the walkers moved by at most one unit in the last place:
    the largest change of weight, overlap, energies and phi of any walker, relative to max(1, |value|)."""
    run = run_oracle(name)
    model, phis, weights, xi, eshift, extra = run['case']
    rng = numpy.random.RandomState(0)
    worst = 0.0
    for _ in range(draws):
        moved = phis * (1.0 + numpy.finfo(float).eps * rng.choice([-1.0, 0.0, 1.0], size=phis.shape))
        walkers = new_walkers(model, moved, weights, extra['ehyb0'])
        for w, e in zip(walkers, extra['ehyb0']):
            w['eloc'] = complex(e)
        for a, b in zip(oracle_step(model, walkers, xi, eshift, extra['hybrid'], extra['cap']), run['verdicts'][0]):
            assert a['live'] == b['live'] and (a['weight'] == 0.0) == (b['weight'] == 0.0), name
            for k in ('weight', 'ot', 'hybrid_energy', 'eloc', 'phi'):
                d = float(numpy.max(numpy.abs(numpy.asarray(a[k]) - numpy.asarray(b[k]))))
                worst = max(worst, d / max(1.0, float(numpy.max(numpy.abs(b[k])))))
    return worst


def check_case(name, case, verdicts):
    """The conditions a case must meet on the reference alone (not tolerances): no marginal decision in either step,
    the coverage of the branches in the first one, dead walkers present.  Returns the first step's summary."""
    model, phis, weights, xi, eshift, extra = case
    s = summary(verdicts[0])
    for n, vs in enumerate(verdicts):
        t = summary(vs)
        assert t['margin_fb'] > GUARD and t['margin_e'] > GUARD and t['margin_cos'] > GUARD, (name, n, t)
        assert t['margin_arg'] > GUARD, (name, n, t)             # (log(ratio) is nowhere on its branch cut)
        # nobody enters the next step with a weight near the 1e-8 below which the driver stops propagating (the parked
        # 5e-9 walker aside)
        wts = numpy.array([abs(v['weight']) for v in vs])
        assert n == len(verdicts) - 1 or not numpy.any((wts > 1e-9) & (wts < 1e-7) & (wts != 5e-9)), (name, n, wts)
    assert 0 < s['live'] < s['nw'] and numpy.count_nonzero(weights == 0.0) >= 1, (name, s)
    checks = extra['checks']
    if 'fb' in checks:
        assert 0.1 * s['pairs'] <= s['clipped'] <= 0.9 * s['pairs'], (name, s)
        assert s['walkers_mixed'] >= 1 and s['walkers_unclipped'] >= 1, (name, s)
    if 'ebound' in checks:
        assert min(s['above'], s['below'], s['inside']) >= 2, (name, s)
    if 'kill' in checks:
        assert s['killed'] >= 0.2 * s['live'] and s['survived'] >= 0.2 * s['live'], (name, s)
    if 'unbounded' in checks:
        assert abs(eshift) >= 1e-10 and s['above'] == s['below'] == 0, (name, s)
    if abs(eshift) < 1e-10:
        assert s['nhe'] == 0, (name, s)
    if extra['overflow']:
        live = [i for i, v in enumerate(verdicts[0]) if v['live']]
        inf = [i for i in live if extra['ehyb0'][i].real == -1e6]
        zero = [i for i in live if extra['ehyb0'][i].real == 1e6]
        assert len(inf) >= 2 and len(zero) >= 2 and len(live) - len(inf) - len(zero) >= 2, (name, inf, zero)
        assert all(verdicts[0][i]['weight'] == 0.0 for i in inf + zero), name
    return s


# ---------------------------------------------------------------------------------------------------------------------
# the cases: one per code path of the step (tests/test_gpu_constraint_edges.py says which kernel each must take)
# ---------------------------------------------------------------------------------------------------------------------
def _generic(M, K, na, nb, closed=False, dt=0.4, top=100.0):
    return dict(kind='generic', M=M, K=K, na=na, nb=nb, dt=dt, closed=closed, top=top)


def _hubbard(nx, ny, na, nb, spin, U=8.0, dt=0.1):
    return dict(kind='hubbard', nx=nx, ny=ny, na=na, nb=nb, U=U, spin=spin, dt=dt)


TINY = _generic(37, 9, 7, 6)
WGJ = _generic(40, 10, 9, 9, closed=True)
SMALL = _generic(12, 12, 3, 3, closed=True)
MSD = dict(kind='msd', M=20, K=8, na=3, nb=2, ndet=3, dt=0.4, top=160.0)
HUB_CHARGE = _hubbard(3, 3, 5, 4, False)
HUB_SPIN = _hubbard(4, 2, 3, 1, True)
UEG = dict(kind='ueg', rs=8.0, na=7, nb=7, ecut=1.0, dt=128.0)
P = dict(amax=0.5, xi_big=2.0)
H = dict(amax=3.0, xi_big=3.0)
# generic Hamiltonians, one determinant: four of the five kernels the weight update is inlined into (the fifth: ``tail-*``)
_case('tiny-open', model=TINY, nw=20, eshift=-100.0, kernels=('greens_tiny_kernel', 'prop_fused_kernel'), **P)
_case('tiny-open-noshift', model=TINY, nw=20, eshift=0.0, checks=('fb', 'kill'), kernels=('greens_tiny_kernel',), **P)
_case('wgj-closed', model=WGJ, nw=33, eshift=-85.0, closed=True, bp=2,
      kernels=('greens_small_kernel<true, true>', 'prop_fused_kernel'), **P)
_case('unfused', model=_generic(130, 8, 5, 4, top=200.0), nw=20, eshift=-67.6, kernels=('greens_kernel', 'weight_kernel'),
      absent=('prop_fused_kernel',), **P)
_case('lds-gj', model=_generic(48, 10, 33, 33, top=50.0), nw=20, eshift=-84.1,
      kernels=('greens_small_kernel<true, false>',), **P)
_case('bigdet', model=_generic(64, 12, 46, 46, top=50.0), nw=20, eshift=-116.5, kernels=('det_combine_kernel',), **P)
# multi-determinant trial, both force-bias algorithms
_case('msd-per-det', model=MSD, nw=20, eshift=-206.1, msd_fb_mode=1, kernels=('weight_kernel',), absent=('msd_gbar',),
      amax=0.6, xi_big=2.0)
_case('msd-gbar', model=MSD, nw=20, eshift=-206.1, msd_fb_mode=2, kernels=('weight_kernel', 'msd_gbar'), amax=0.6,
      xi_big=2.0)
# populations on both sides of the 32- and 64-walker tilings, and one past 256
for _nw, _es in ((32, -185.8), (33, -131.0), (64, -126.2), (65, -161.9)):
    _case('nw-%d' % _nw, model=SMALL, nw=_nw, eshift=_es, closed=True, kernels=('greens_tiny_kernel',), **P)
_case('nw-257', model=_generic(10, 6, 2, 2, closed=True), nw=257, eshift=-44.8, closed=True,
      kernels=('greens_tiny_kernel',), **P)
# fields drawn on the device
_case('philox-generic', model=TINY, nw=20, eshift=-125.0, philox=(2024, 3), kernels=('greens_tiny_kernel',), **P)
_case('philox-hubbard', model=HUB_CHARGE, nw=33, eshift=30.5, philox=(77, 1), kernels=('fields_kernel<true>',), **H)
# plane waves, lattice models
_case('ueg', model=UEG, nw=20, eshift=-0.6, kernels=('ueg_',), amax=1.0, xi_big=2.0)
_case('hubbard-charge', model=HUB_CHARGE, nw=33, eshift=19.9, kernels=('fields_kernel<true>',), **H)
_case('hubbard-charge-noshift', model=HUB_CHARGE, nw=33, eshift=0.0, checks=('fb', 'kill'),
      kernels=('fields_kernel<true>',), **H)
_case('hubbard-spin', model=HUB_SPIN, nw=20, eshift=-8.9, kernels=('fields_kernel<true>',), **H)
# local-energy weights
_case('local-energy-generic', model=TINY, nw=20, eshift=-13.9, hybrid=False, kernels=('greens_tiny_kernel',), **P)
_case('local-energy-hubbard', model=HUB_CHARGE, nw=33, eshift=1.0, hybrid=False, kernels=('fields_kernel<true>',), **H)
# the weight cap behind a phase kill
_case('cap', model=TINY, nw=20, eshift=-100.0, cap=(0.02, 20.0), kernels=('greens_tiny_kernel',), **P)
# infinite and vanishing importance functions, no bound
_case('overflow', model=TINY, nw=20, eshift=0.0, overflow=True, bp=2, checks=('fb',), kernels=('greens_tiny_kernel',), **P)
# the headline shape with energies the bound leaves alone
C3 = dict(amax=0.1, xi_big=1.0, checks=('unbounded',))
_case('c3-closed', model=_generic(100, 12, 25, 25, closed=True, dt=0.01, top=0.0), nw=16, eshift=-130.0, closed=True,
      closed_deal=True, kernels=('greens_small_kernel<true, true>', 'prop_fused_kernel'), **C3)
_case('c3-open', model=_generic(100, 12, 25, 25, dt=0.01, top=0.0), nw=16, eshift=-52.0,
      kernels=('greens_small_kernel<true, true>', 'prop_fused_kernel'), **C3)
# the shape class whose steps close as the tail of the fused propagator's launch (k_step_fusion_shape: real RHF trial, one
# real BH1, na == nb in 17..32, M in 97..104) with more than 32 walkers (the spin-sum force bias): its corners -- 25 and 26
# k-steps, the emptiest and the fullest second column slot, row tile 6 with 4, 1 and 8 live rows.  Unannounced steps in the
# default scope run the two launches (tests/test_gpu_constraint_edges.py); tests/test_gpu_constraint_tail.py takes the same
# populations through the tail on every route to it.  ``mixed``: open walkers beside resident ones in the same launch;
# ``tail-bp``: a back-propagation window, with which no step may fuse.
def _tail(M, N):
    return _generic(M, 12, N, N, closed=True)


TAIL = dict(closed=True, kernels=('greens_small_kernel<true, true>', 'prop_fused_kernel'),
            absent=('prop_fused_kernel<false, 7, true',), **P)
_case('tail-100-25', model=_tail(100, 25), nw=33, eshift=-224.6, closed_deal=True, **TAIL)
_case('tail-97-17', model=_tail(97, 17), nw=33, eshift=-158.2, closed_deal=True, **TAIL)
_case('tail-104-32', model=_tail(104, 32), nw=33, eshift=-261.9, closed_deal=True, **TAIL)
_case('tail-cap', model=_tail(100, 25), nw=65, eshift=-212.2, cap=(0.02, 60.0), closed_deal=True, **TAIL)
_case('tail-philox', model=_tail(100, 25), nw=33, eshift=-183.5, philox=(2024, 3), closed_deal=True, **TAIL)
_case('tail-overflow', model=_tail(100, 25), nw=33, eshift=0.0, overflow=True, checks=('fb',), closed_deal=True, **TAIL)
_case('tail-mixed', model=_tail(100, 25), nw=33, eshift=-202.3, mixed=True, **TAIL)
_case('tail-bp', model=_tail(100, 25), nw=33, eshift=-224.6, bp=2, closed_deal=True, **TAIL)
# the cases of the shape class whose steps fuse (everything but the back-propagation window)
TAIL_FUSING = ('tail-100-25', 'tail-97-17', 'tail-104-32', 'tail-cap', 'tail-philox', 'tail-overflow', 'tail-mixed')
