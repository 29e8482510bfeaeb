"""Lattices on which the direct update, the free projection and the back-propagation of the discrete Hirsch fields are held
to the oracle (tests/test_gpu_hirsch_paths.py), with the oracle's result of every case.

The three paths (propagation/hubbard.py:222-275, 303-343, 568-672) take their inverse overlaps from the routine that
dispatches on the electron count (registers up to 32 per spin, LDS up to 45, the blocked Gauss-Jordan above), the direct
update walks the sites in chunks of 256, and the one-body products go through another engine for M > 128 with 64 walkers or
more: the lattices below sit on both sides of each of these.

Models and populations are built as ``run_hirsch_lattice`` of tests/test_gpu_fullsize.py builds them: ``systems.Hubbard``
(U = 4), ``uhf_trial_hubbard(ueff=0.4)``, ``ref.HirschModel`` (dt = 0.01), walkers psi + 0.02 noise, weights cycling through
1.0, 0.7, 0.0, 1.3.  On top of that:

  * direct update: walker FLIPPED tracks minus its true overlap, so the first kinetic step kills it; a case with ``kill``
    names a walker whose uniforms are all 0: every site takes field 0, phi is scaled by one factor, and the ratio the direct
    update tests has the phase Im(gamma) (N_e - M) whatever the walker is -- 2.2 rad on 6 x 6 with 13 + 12 electrons in the
    charge decomposition, beyond pi / 2.  ``balanced`` cases give every other walker as many fields 0 as 1 (in a random
    arrangement): the charge decomposition chooses with probability 1/2 whatever the walker is, and away from half filling
    the phase of the ratio would otherwise be a random walk over the sites that kills by chance.
  * free projection: walker PARKED has weight 5e-9, below the 1e-8 at which the driver stops propagating.
  * back-propagation: walker SRC is copied over walker DST in mid-window, walker DEAD starts dead and is given a weight
    in mid-window (a walker whose recorded history is shorter than the others' and still counts), the other walkers with
    weight 0 stay dead.

``run_direct`` / ``run_free`` / ``run_bp`` return what the oracle makes of a case, computed once per session; nobody may change
what they return.  ``check_direct`` asserts, on the oracle alone, that no decision of a case is marginal: a seed that misses
this fails in tests/test_hirsch_paths_cpu.py as a fixture error, never as a device mismatch.
"""
import cmath
import copy
import functools
import math

import numpy

from oracle import afqmc_ref as ref
from pauxy_amd import systems, trial as trial_mod

try:                                    # the oracle's matrices are small: a BLAS thread pool only gets in their way
    from threadpoolctl import threadpool_limits
except ImportError:
    threadpool_limits = None


def one_thread(f):
    @functools.wraps(f)
    def g(*a):
        if threadpool_limits is None:
            return f(*a)
        with threadpool_limits(limits=1):
            return f(*a)
    return g


U, DT, ESHIFT = 4.0, 0.01, 0.3
THRESHOLD_GUARD = 1e-6      # no uniform of a live walker is closer to the probability it is compared with
ARG_GUARD = 0.2             # rad: distance of arg(ratio) of the direct update from pi / 2, on either side
WEIGHTS = (1.0, 0.7, 0.0, 1.3)
FLIPPED, DEAD, PARKED = 1, 2, 1
SRC, DST, REVIVED_WEIGHT = 0, 3, 0.9

L2, L3, L42, L6, L9, L12, L17 = ((2, 2, 2, 2), (3, 3, 5, 4), (4, 2, 3, 0), (6, 6, 18, 17), (9, 9, 40, 33), (12, 12, 72, 70),
                                 (17, 16, 20, 19))

# name -> lattice (nx, ny, na, nb), decomposition, walkers
DIRECT = {
    '2x2-spin': dict(lat=L2, charge=False, nw=5),                  # one partial chunk, tiny N
    '3x3-charge': dict(lat=L3, charge=True, nw=7),                 # odd M, unequal spins
    '4x2-spin-nobeta': dict(lat=L42, charge=False, nw=4),          # empty beta spin
    '6x6-charge': dict(lat=L6, charge=True, nw=9),
    '9x9-spin': dict(lat=L9, charge=False, nw=4),                  # LDS Gauss-Jordan on alpha, registers on beta
    '12x12-spin-64': dict(lat=L12, charge=False, nw=64),           # blocked Gauss-Jordan, ring engine with dead walkers
    '17x16-charge': dict(lat=L17, charge=True, nw=3, balanced=True),   # second, ragged chunk of 16 sites
    '17x16-spin': dict(lat=L17, charge=False, nw=3),
    '6x6-charge-kill': dict(lat=(6, 6, 13, 12), charge=True, nw=6, balanced=True, kill=3),
    '3x3-charge-logshift': dict(lat=L3, charge=True, nw=7, log_shift=0.9),
}
FREE = {
    '2x2-spin': dict(lat=L2, charge=False, nw=5),
    '3x3-charge': dict(lat=L3, charge=True, nw=7),
    '9x9-spin': dict(lat=L9, charge=False, nw=4),
    '12x12-spin-64': dict(lat=L12, charge=False, nw=64),
    '17x16-charge': dict(lat=L17, charge=True, nw=3),
    '17x16-spin': dict(lat=L17, charge=False, nw=3),
    '3x3-charge-logshift': dict(lat=L3, charge=True, nw=7, log_shift=0.9),
}
# window length, stabilisation period, steps after which the copy / the revival happen, length of the second window
BP = {
    '3x3-spin': dict(lat=L3, charge=False, nw=7, nbp=5, nstblz=2, copy_after=2, revive_after=1, nbp2=3),
    '6x6-charge': dict(lat=L6, charge=True, nw=9, nbp=4, nstblz=3, copy_after=1, revive_after=0, nbp2=2),
    '12x12-spin-64': dict(lat=L12, charge=False, nw=64, nbp=2, nstblz=5, copy_after=0, revive_after=0, nbp2=1),
}


@functools.lru_cache(maxsize=None)
@one_thread
def model(lat, charge, log_shift=0.0):
    nx, ny, na, nb = lat
    s = systems.Hubbard(nx, ny, na, nb, U)
    t = trial_mod.uhf_trial_hubbard(s, ueff=0.4)
    m = ref.HirschModel(s.T.astype(complex), U, numpy.array(t.psi), na, nb, DT, charge)
    if log_shift:
        m.log_shift = log_shift
    return m


def case_model(spec):
    return model(spec['lat'], spec['charge'], spec.get('log_shift', 0.0))


def population(m, nw, seed=9):
    rng = numpy.random.RandomState(seed)
    nt = m.na + m.nb
    phis = numpy.array([m.psi + 0.02 * (rng.rand(m.M, nt) + 1j * rng.rand(m.M, nt)) for _ in range(nw)])
    return rng, phis, numpy.resize(numpy.array(WEIGHTS), nw)


def balanced_uniforms(rng, M):
    """Uniforms that choose field 0 on one half of the sites (a random half) and field 1 on the other, none near 1/2."""
    f = numpy.ones(M, dtype=int)
    f[rng.permutation(M)[:M // 2]] = 0
    return numpy.where(f == 0, 0.05, 0.55) + 0.4 * rng.rand(M)


def direct_probabilities(m, phi):
    """pp / norm of every site, the number a uniform is compared with in two_body_direct (hubbard.py:246-252)."""
    G = ref.greens_function(phi, m.psi, m.na, m.nb)[2]
    nia, nib = G[0].diagonal(), G[1].diagonal()
    fb = nia + nib - 1 if m.charge else nia - nib
    pp, pm = 0.5 * numpy.exp(m.gamma * fb).real, 0.5 * numpy.exp(-m.gamma * fb).real
    return pp / (pp + pm)


def snapshot(walkers):
    return dict(phi=numpy.array([w['phi'] for w in walkers]), weight=numpy.array([float(w['weight']) for w in walkers]),
                ot=numpy.array([complex(w['ot']) for w in walkers]),
                phase=numpy.array([complex(w['phase']) for w in walkers]))


def build_direct(name):
    """-> (model, phis, weights, ot0, u): ot0 is what the device is told to track (minus the overlap for FLIPPED)."""
    spec = DIRECT[name]
    m = case_model(spec)
    rng, phis, w0 = population(m, spec['nw'])
    u = rng.rand(spec['nw'], m.M)
    if spec.get('balanced'):
        u = numpy.array([balanced_uniforms(rng, m.M) for _ in range(spec['nw'])])
    if 'kill' in spec:
        u[spec['kill']] = 0.0
    ot0 = numpy.array([m.overlap(p) for p in phis])
    ot0[FLIPPED] = -ot0[FLIPPED]
    return m, phis, w0, ot0, u


@functools.lru_cache(maxsize=None)
@one_thread
def run_direct(name):
    """The three calls of a step with ``single_site_update: False`` (propagate_walker_constrained, hubbard.py:285-312, for the
    walkers the driver propagates, |weight| > 1e-8): -> dict(case, kinetic, two_body, finish: snapshots after each call,
    fields [nw, M] (-1: not updated), used [nw], gap [nw]: min over the sites of |u - pp / norm|, arg [nw]: the phase of the
    ratio the direct update tested (nan: the walker did not get there))."""
    m, phis, w0, ot0, u = case = build_direct(name)
    nw, M = len(w0), m.M
    walkers = [ref.new_walker(m, p, weight=float(w)) for p, w in zip(phis, w0)]
    for wk, o in zip(walkers, ot0):
        wk['ot'] = complex(o)
    live = numpy.abs(w0) > 1e-8
    for wk, l in zip(walkers, live):
        if l:
            ref.hirsch_kinetic_importance_sampling(m, wk)
    out = dict(case=case, kinetic=snapshot(walkers), fields=-numpy.ones((nw, M), dtype=int), used=numpy.zeros(nw, dtype=int),
               gap=numpy.full(nw, numpy.inf), arg=numpy.full(nw, numpy.nan))
    for i, wk in enumerate(walkers):
        if live[i] and abs(wk['weight']) > 0:
            out['gap'][i] = numpy.min(numpy.abs(u[i] - direct_probabilities(m, wk['phi'])))
            ot_before = wk['ot']
            it = iter(u[i])
            f = ref.hirsch_two_body_direct(m, wk, lambda: next(it))
            wfac = 1.0 + 0j
            for x in f:
                wfac *= m.aux_wfac[x]
            out['arg'][i] = cmath.phase(wfac * m.overlap(wk['phi']) / ot_before)
            out['fields'][i], out['used'][i] = f, M
    out['two_body'] = snapshot(walkers)
    for wk, l in zip(walkers, live):
        if l:
            if abs(numpy.real(wk['weight'])) > 0:
                ref.hirsch_kinetic_importance_sampling(m, wk)
            wk['weight'] *= numpy.exp(m.dt * ESHIFT)
    out['finish'] = snapshot(walkers)
    return out


def check_direct(name, run):
    """What a direct case must be on the oracle alone: a dead walker, the FLIPPED walker killed by the first kinetic step and
    nobody else by either, no uniform within THRESHOLD_GUARD of its probability, every ratio the direct update tests at least
    ARG_GUARD inside pi / 2 -- but the named walker's, which is at least as far beyond it and the only one killed."""
    m, phis, w0, ot0, u = run['case']
    spec = DIRECT[name]
    live = numpy.abs(w0) > 1e-8
    assert w0[DEAD] == 0.0 and live[FLIPPED]
    entered = live & (run['kinetic']['weight'] != 0.0)
    assert list(numpy.nonzero(live & ~entered)[0]) == [FLIPPED], name
    assert entered.sum() >= 1
    assert numpy.all(run['gap'][entered] >= THRESHOLD_GUARD), (name, run['gap'])
    killed = spec.get('kill')
    for i in numpy.nonzero(entered)[0]:
        a = abs(run['arg'][i])
        if i == killed:
            assert 0.5 * math.pi + ARG_GUARD <= a <= math.pi and run['two_body']['weight'][i] == 0.0, (name, i, a)
            assert numpy.all(run['fields'][i] == 0)
        else:
            assert a <= 0.5 * math.pi - ARG_GUARD and run['two_body']['weight'][i] != 0.0, (name, i, a)
            assert run['finish']['weight'][i] != 0.0, (name, i)                 # (nor does the second kinetic step kill)
    assert numpy.all(run['fields'][~entered] == -1) and numpy.all(run['used'][~entered] == 0)
    assert numpy.all(run['used'][entered] == m.M) and numpy.all(run['fields'][entered] >= 0)


def build_free(name):
    spec = FREE[name]
    m = case_model(spec)
    rng, phis, w0 = population(m, spec['nw'], seed=10)
    w0[PARKED] = 5e-9
    u = rng.rand(2, spec['nw'], m.M)
    assert numpy.min(numpy.abs(u - 0.5)) > 1e-9
    return m, phis, w0, numpy.array([m.overlap(p) for p in phis]), u


@functools.lru_cache(maxsize=None)
@one_thread
def run_free(name):
    """Two steps of propagate_walker_free (hubbard.py:303-343) for the walkers with |weight| > 1e-8: -> dict(case, steps:
    [snapshot + fields [nw, M] (-1: not propagated)] * 2)."""
    m, phis, w0, ot0, u = case = build_free(name)
    walkers = [ref.new_walker(m, p, weight=float(w)) for p, w in zip(phis, w0)]
    steps = []
    for us in u:
        fields = -numpy.ones((len(w0), m.M), dtype=int)
        for i, wk in enumerate(walkers):
            if abs(wk['weight']) > 1e-8:
                it = iter(us[i])
                fields[i] = ref.propagate_walker_hirsch_free(m, wk, lambda: next(it), ESHIFT)
        steps.append(dict(snapshot(walkers), fields=fields))
    return dict(case=case, steps=steps)


def build_bp(name):
    spec = BP[name]
    m = case_model(spec)
    rng, phis, w0 = population(m, spec['nw'], seed=11)
    u = rng.rand(spec['nbp'] + spec['nbp2'], spec['nw'], m.M)
    return m, phis, w0, numpy.array([m.overlap(p) for p in phis]), u, spec


@functools.lru_cache(maxsize=None)
@one_thread
def run_bp(name):
    """Two windows of single-site steps (nbp, then nbp2 of them) with the one_rdm estimator of
    estimators/back_propagation.py:127-226 at the end of each: -> dict(case, fields [step][nw, M], weights [step][nw],
    steps: bp_steps before each update, est: [3 energies, denominator, G.flatten()] of each)."""
    m, phis, w0, ot0, u, spec = case = build_bp(name)
    nw, M = spec['nw'], m.M
    walkers = [ref.new_walker(m, p, weight=float(w)) for p, w in zip(phis, w0)]
    for wk in walkers:
        wk['bp'] = ref.bp_new(M, spec['nbp'])
        wk['phi_old'] = wk['phi'].copy()
    out = dict(case=case, fields=[], weights=[], steps=[], est=[])
    step = 0
    for window, n in enumerate((spec['nbp'], spec['nbp2'])):
        for k in range(n):
            fields = -numpy.ones((nw, M), dtype=int)
            for i, wk in enumerate(walkers):
                if abs(wk['weight']) > 1e-8:
                    it = iter(u[step][i])
                    f = ref.propagate_walker_hirsch(m, wk, lambda: next(it), ESHIFT)
                    if f is not None:
                        fields[i, :len(f)] = f
            out['fields'].append(fields)
            out['weights'].append(numpy.array([float(wk['weight']) for wk in walkers]))
            step += 1
            if window == 0 and k == spec['revive_after']:
                walkers[DEAD]['weight'] = REVIVED_WEIGHT
            if window == 0 and k == spec['copy_after']:
                walkers[DST] = copy.deepcopy(walkers[SRC])
        out['steps'].append(numpy.array([wk['bp']['step'] for wk in walkers]))
        est = numpy.zeros(4 + 2 * M * M, dtype=complex)
        ref.bp_update(m, walkers, spec['nstblz'], est)
        out['est'].append(est)
    return out
