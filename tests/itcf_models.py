"""Model builders of the ITCF GPU tests and of tools/itcf_bench.py: a Generic system with its device handle inputs,
and a device handle with the discrete Hirsch propagator on a Hubbard lattice; and the comparison every ITCF GPU test
makes: the device's window sums against the extended-precision restatement of the recorded histories, under the rule
of tests/itcf_ref_ext.py (bound)."""
import math
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy
import scipy.linalg

from pauxy_amd import _lib as L, systems, trial as trial_mod
from pauxy_amd.device import AfqDevice
from pauxy_amd.propagation import setup
from oracle import afqmc_ref as ref
from tests import itcf_ref, itcf_ref_ext as X


def generic_model(M, K, na, nb, seed=3, dt=0.01, hermitian=False, rhf=False):
    """A Generic system with symmetric real (or, hermitian=True, Hermitian complex) Cholesky vectors, its trial and
    propagator arrays.  rhf: the closed-shell real trial (the lowest na = nb orbitals of h1e in both spins, spin blocks
    bitwise equal) instead of the perturbed complex open-shell one."""
    rng = numpy.random.RandomState(seed)
    h = rng.normal(size=(M, M))
    h1e = 0.5 * (h + h.T) - 2.0 * numpy.eye(M)
    A = rng.normal(size=(K, M, M)) * (0.3 / numpy.sqrt(M))
    if hermitian:
        A = A + 1j * rng.normal(size=(K, M, M)) * (0.3 / numpy.sqrt(M))
        Lv = 0.5 * (A + A.conj().transpose(0, 2, 1))
    else:
        Lv = 0.5 * (A + A.transpose(0, 2, 1))
    chol = numpy.ascontiguousarray(Lv.reshape(K, M * M).T)
    s = systems.Generic((na, nb), numpy.array([h1e, h1e]), chol, ecore=0.1)
    e, v = numpy.linalg.eigh(h1e)
    psi = numpy.zeros((M, na + nb), dtype=complex)
    psi[:, :na] = v[:, :na]
    psi[:, na:] = v[:, :nb]
    if rhf:
        assert na == nb
    else:
        psi = psi + 0.05 * (rng.rand(M, na + nb) + 1j * rng.rand(M, na + nb))
    t = trial_mod.SingleDetTrial(s, psi)
    BH1, mf = setup.generic_propagator_arrays(s, t, dt)
    model = ref.RefModel('generic', M, na, nb, t.psi, BH1, mf, dt, hs_pot=s.hs_pot, rchol=t._rchol,
                         H1=s.H1.astype(complex), ecore=0.1)
    return model, s, rng


def hirsch_device(nx, ny, na, nb, nw, U=4.0, dt=0.05, seed=4, charge_decomposition=False):
    """A device with the discrete Hirsch propagator (spin or charge decomposition) on an nx x ny Hubbard model and nw
    perturbed trial walkers."""
    s = systems.Hubbard(nx, ny, na, nb, U)
    M = nx * ny
    T = numpy.asarray(s.T, dtype=complex)
    BT2 = numpy.array([scipy.linalg.expm(-0.5 * dt * T[i]) for i in range(2)])
    e, v = numpy.linalg.eigh(T[0].real)
    rng = numpy.random.RandomState(seed)
    psi = numpy.hstack([v[:, :na], v[:, :nb]]).astype(complex)
    dev = AfqDevice(0)
    dev.set_system_hubbard(T, U, na, nb)
    dev.set_trial(psi)
    dev.set_propagator_hirsch(BT2, dt, charge_decomposition)
    dev.walkers_alloc(nw)
    ne = na + nb
    dev.set(L.F_PHI, numpy.array([psi + 0.05 * rng.rand(M, ne) for _ in range(nw)]))
    dev.set(L.F_OT, dev.calc_overlap())
    return dev, BT2, psi, rng, U, dt


def restore_factors(dev, psi, nstblz):
    """weight_w (phase product / cosine product) per walker: the back-propagation's 'full' denominator of one walker."""
    w0 = dev.get(L.F_WEIGHT).copy()
    out = numpy.zeros(dev.nw, dtype=complex)
    for i in range(dev.nw):
        if w0[i] == 0:
            continue
        one = numpy.zeros(dev.nw)
        one[i] = 1.0
        dev.set(L.F_WEIGHT, one)
        out[i] = w0[i] * dev.bp_update(psi, nstblz, 'full', reset=False)[1]
    dev.set(L.F_WEIGHT, w0)
    return out


# seconds of one core per walker, step and M^3 of the extended restatement (numpy's own loops for longdouble)
EXT_COST = 2.5e-7
SAMPLE = 4


def extended_sums(kind, model, fields, phi0, psi_T, na, nmax, nstblz, stable, wfac, walkers):
    """The extended restatement's window sums over ``walkers``; worker processes (fresh interpreters that import numpy
    alone and never open the device) share a population whose restatement would take one core more than four seconds by
    EXT_COST.  Those are the cases with M >= 64 and more than a few walker-steps: M = 64 with 33 / 64 / 65 walkers (6 ..
    13 s on one core), M = 100 with 8 or 33 walkers (8 / 25 s), M = 97 .. 128 with 3 .. 5 walkers, the 13+9 cases at
    M = 100 -- about 100 s of one core together, against 60 s for the whole of the three ITCF files with the pool.  Every
    M <= 48 case, the 257- and 1000-walker ones included, runs in this process in chunks.  Without those cases the pool
    (nproc, the executor, EXT_COST) can go and the chunk loop alone remains."""
    M = phi0.shape[-2]
    if not len(walkers):
        return numpy.zeros((nmax + 1, 2, 2, M, M), dtype=X.CLD)
    cost = EXT_COST * len(fields) * M ** 3 * len(walkers)
    nproc = min(12, len(walkers)) if cost > 4.0 else 1
    per = int(math.ceil(len(walkers) / float(nproc)))
    if nproc == 1:
        per = min(per, max(1, int(2 ** 26 // (len(fields) * M * M))))          # 2 GB of B matrices at most
    chunks = [walkers[i:i + per] for i in range(0, len(walkers), per)]
    args = [(kind, model, fields[:, c], phi0[c], psi_T, na, nmax, nstblz, stable, wfac[c]) for c in chunks]
    if nproc == 1:
        parts = [X.window_sums(*a) for a in args]
    else:
        with ProcessPoolExecutor(nproc, mp_context=multiprocessing.get_context('spawn')) as pool:
            parts = list(pool.map(X.window_sums, *zip(*args)))
    return sum(parts[1:], parts[0])


def compare_window(case, got, kind, model, fields, phi0, psi_T, na, nmax, nstblz, stable, wfac, sample=False, path=''):
    """The rule of tests/itcf_ref_ext.py on one window: got = (spgf, den) of afq_itcf_update, fields [n, nw, ...] the
    recorded history, phi0 the walkers at the window start, wfac the weight of each walker in the window (0: none).

    err_ref is the largest slice error of the fp64 restatement's sums against the extended restatement's; the device
    passes when every slice of its sums is within bound(err_ref) of the extended sums.  sample (M >= 100 with 64 or
    more walkers only: the extended restatement of the population would take minutes): err_ref from SAMPLE live walkers
    (first, last and those between) and the device against the fp64 restatement's sums under the same bound."""
    spgf, den = got
    nw, M = phi0.shape[0], phi0.shape[-2]
    wfac = numpy.asarray(wfac, dtype=complex)
    live = [w for w in range(nw) if wfac[w] != 0]
    assert not sample or (M >= 100 and nw >= 64), "only M >= 100 with 64 or more walkers may be sampled"
    use = live
    if sample and len(live) > SAMPLE:
        use = [live[(len(live) - 1) * k // (SAMPLE - 1)] for k in range(SAMPLE)]

    def b64(w):
        if kind == 'generic':
            return numpy.array([itcf_ref.b_generic(model[0], model[1], x[w], model[2]) for x in fields])
        return numpy.array([itcf_ref.b_hirsch(model[0], x[w], model[1], model[2]) for x in fields])
    wins = {w: itcf_ref.window(b64(w), phi0[w], psi_T, na, nmax, nstblz, stable) for w in (live if sample else use)}
    zero = numpy.zeros((nmax + 1, 2, 2, M, M))
    sums64 = itcf_ref.accumulate([wins[w] for w in use], wfac[use]) if use else zero
    sumsx = extended_sums(kind, model, numpy.asarray(fields), phi0, psi_T, na, nmax, nstblz, stable, wfac, use)
    err_ref = float(numpy.max(X.slice_errors(sums64, sumsx)))
    limit = X.bound(err_ref)
    want = sumsx
    if sample and len(live) > SAMPLE:
        want = itcf_ref.accumulate([wins[w] for w in live], wfac[live])
    err = X.slice_errors(spgf, want)
    worst = float(numpy.max(err))
    print("ITCF-CASE | %s | M=%d nw=%d live=%d nmax=%d n=%d %s | err_ref %.2e | device %.2e | bound %.2e | ratio %.3f | %s | %s"
          % (case, M, nw, len(live), nmax, len(fields), 'stable' if stable else 'unstable', err_ref, worst, limit,
             worst / limit, 'sampled %d, device vs fp64' % SAMPLE if want is not sumsx else 'extended', path))
    den_want = complex(numpy.sum(wfac))
    assert abs(den - den_want) <= 1e-12 * max(1.0, abs(den_want)), (den, den_want)
    assert numpy.isfinite(spgf).all()
    # a model whose fp64 restatement is already this far off is badly conditioned: change the model, not the rule
    assert err_ref <= 1e-13, err_ref
    assert worst <= limit, (case, worst, limit, numpy.argwhere(err > limit)[:8].tolist())
    return err_ref, worst, limit
