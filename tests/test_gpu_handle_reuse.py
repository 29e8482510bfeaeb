"""A handle that has served other configurations gives bitwise the results of a fresh handle.

One long-lived AfqDevice walks through systems, trials and population sizes that grow and shrink (so that a buffer
kept from an earlier configuration would be overrun or misread); after every stage the same stage runs on a fresh
handle with the same seed, and every walker field and energy must be equal bit for bit.  This is what holds the
release of device memory by lifetime (csrc/dev_mem.h) to account."""
import numpy
import pytest
import scipy.linalg

from pauxy_amd import _lib as L
from pauxy_amd import systems, trial as trial_mod
from pauxy_amd.device import AfqDevice
from pauxy_amd.propagation import setup
from tests.helpers import ueg_model

pytestmark = pytest.mark.gpu
FIELDS = (('phi', L.F_PHI), ('weight', L.F_WEIGHT), ('ot', L.F_OT), ('ghalf', L.F_GHALF))


def perturbed(psi, nw, seed):
    rng = numpy.random.RandomState(seed)
    return numpy.array([psi + 0.05 * (rng.rand(*psi.shape) + 1j * rng.rand(*psi.shape)) for _ in range(nw)])


def measure(dev, psi, nw, step, reortho=False, window=None):
    """One greens, one local_energy, two steps (four and the window's update with window); -> every compared array."""
    dev.rng_seed(7)
    dev.set(L.F_PHI, perturbed(psi, nw, 11))
    dev.set(L.F_OT, dev.calc_overlap())
    out = {'ot0': dev.greens(), 'energy': dev.local_energy()}
    if window:
        dev.bp_configure(window)
    else:
        with pytest.raises(L.AfqError) as e:                # "not configured", whatever the handle did before
            dev.bp_update(psi, 5)
        assert e.value.code == -2
    rng = numpy.random.RandomState(13)
    for _ in range(window or 2):
        step(dev, rng)
    if window:
        E, den, G = dev.bp_update(psi, 5, eval_energy=True)
        out.update(bp_E=E, bp_den=numpy.array(den), bp_G=G)
    if reortho:
        out['detR'] = dev.reortho()
    for name, f in FIELDS:
        out[name] = dev.get(f)
    out['energy2'] = dev.local_energy()
    return out


def continuous(dev, rng):
    dev.propagate(rng.normal(size=(dev.nw, dev.K)), 0.1)


def hirsch(dev, rng):
    dev.propagate_hirsch(0.1)


def hubbard(nx, ny, ne, seed):
    s = systems.Hubbard(nx, ny, ne, ne, 4.0)
    q = numpy.linalg.qr(numpy.random.RandomState(seed).rand(nx * ny, ne))[0]
    T = s.T.astype(complex)
    B = numpy.array([scipy.linalg.expm(-0.005 * T[0]), scipy.linalg.expm(-0.005 * T[1])])
    return T, numpy.hstack([q, q]).astype(complex), B


def stages(golden):
    """(name, what the long-lived handle is told, what a fresh one needs for the same state, measure arguments)"""
    s = systems.synthetic_generic(12, 10, (3, 3), seed=1)
    t = trial_mod.rhf_trial_generic(s)
    BH1, mf = setup.generic_propagator_arrays(s, t, 0.01)
    H1 = s.H1.astype(complex)

    def generic(nw, system=True):
        def go(dev):
            if system:
                dev.set_system_generic(s.hs_pot, t._rchol, H1, 0.0, 3, 3)
                dev.set_trial(t.psi)
                dev.set_propagator(BH1, mf, 0.01)
            dev.walkers_alloc(nw)
        return go
    yield 'generic-4', generic(4), generic(4), dict(psi=t.psi, nw=4, step=continuous, window=4)
    yield 'generic-9', generic(9, system=False), generic(9), dict(psi=t.psi, nw=9, step=continuous)

    # three determinants on the same system: the trial, two rotations of it
    rng = numpy.random.RandomState(5)
    dets = numpy.array([t.psi] + [numpy.hstack([numpy.linalg.qr(t.psi[:, :3] + 0.2 * rng.rand(12, 3))[0]] * 2)
                                  for _ in range(2)]).astype(complex)
    coeffs = numpy.array([0.8, 0.5 + 0.1j, -0.3])
    mt = trial_mod.MultiDetTrial(s, (coeffs, dets))
    BH1m, mfm = setup.generic_propagator_arrays(s, mt, 0.01)
    per = 12 * 6

    def msd(dev):
        dev.set_system_generic(s.hs_pot, mt._rchol[:per], H1, 0.0, 3, 3)
        dev.set_trial_multi(dets, coeffs, mt._rchol)
        dev.set_propagator(BH1m, mfm, 0.01)
        dev.walkers_alloc(5)
    yield 'generic-3det-5', msd, msd, dict(psi=t.psi, nw=5, step=continuous)
    yield 'generic-1det-5', generic(5), generic(5), dict(psi=t.psi, nw=5, step=continuous)

    T, psi, B = hubbard(4, 4, 7, 2)

    def hub_hirsch(dev):
        dev.set_system_hubbard(T, 4.0, 7, 7)
        dev.set_trial(psi)
        dev.set_propagator_hirsch(B, 0.01)
        dev.walkers_alloc(6)

    def hub_cont(dev):
        dev.set_system_hubbard(T, 4.0, 7, 7)
        dev.set_trial(psi)
        dev.set_propagator(B, numpy.zeros(16), 0.01)
        dev.walkers_alloc(6)
    yield 'hubbard-hirsch-6', hub_hirsch, hub_hirsch, dict(psi=psi, nw=6, step=hirsch)
    yield 'hubbard-continuous-6', hub_cont, hub_cont, dict(psi=psi, nw=6, step=continuous)

    m = ueg_model(golden('ueg_ops.npz'), 'U_')

    def ueg(dev):
        dev.set_system_ueg(m.iA, m.iB, m.ikpq_i, m.ikpq_kpq, m.ipmq_i, m.ipmq_pmq, m.vqvec, m.vol, m.H1diag, m.ecore,
                           m.na, m.nb)
        dev.set_trial(m.psi)
        dev.set_propagator(m.BH1, m.mf_shift, m.dt, exp_order=m.exp_order)
        dev.walkers_alloc(4)
    yield 'ueg-4', ueg, ueg, dict(psi=numpy.asarray(m.psi, dtype=complex), nw=4, step=continuous)

    Tb, psib, Bb = hubbard(12, 12, 130, 1)              # N = 130 > 128: the large-determinant kernels

    def big(nw, system=True):
        def go(dev):
            if system:
                dev.set_system_hubbard(Tb, 4.0, 130, 130)
                dev.set_trial(psib)
                dev.set_propagator(Bb, numpy.zeros(144), 0.01)
            dev.walkers_alloc(nw)
        return go
    yield 'hubbard-144-2', big(2), big(2), dict(psi=psib, nw=2, step=continuous, reortho=True)
    yield 'hubbard-144-3', big(3, system=False), big(3), dict(psi=psib, nw=3, step=continuous, reortho=True)
    yield 'generic-4-again', generic(4), generic(4), dict(psi=t.psi, nw=4, step=continuous, window=4)


def same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert numpy.array_equal(a[k], b[k]), (what, k)


def test_reused_handle_equals_fresh_handle(golden):
    used = AfqDevice(0)
    first = None
    for name, configure, configure_fresh, args in stages(golden):
        configure(used)
        got = measure(used, **args)
        fresh = AfqDevice(0)
        try:
            configure_fresh(fresh)
            same(got, measure(fresh, **args), name)
        finally:
            fresh.close()
        assert all(numpy.all(numpy.isfinite(v)) for v in got.values()), name
        first = first or got
    same(got, first, 'the first configuration again')
    used.close()
    used.close()                                            # a second close stays harmless
