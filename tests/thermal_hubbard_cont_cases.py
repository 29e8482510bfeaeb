"""What the CPU and the GPU tests of the Hubbard model with continuous fields share: the fixture
(tests/golden/thermal_hubbard_cont.npz), the project's system and trial of a fixture case, and the restatement
(tests/thermal_hubbard_cont_ref.py) run over a case's fields, once per process and kit."""
import functools
import os

import numpy

from tests import thermal_hubbard_cont_ref as R
from tests.thermal_ueg_ref import Kit64
from tests.thermal_ueg_ref_ext import KitExt

HERE = os.path.dirname(os.path.abspath(__file__))
NA, NB = 8, 2                   # single-walker cases a0 .. a7, driver runs b0, b1
STORED_G = (0, 1, 2, 3, 4, 5)   # the cases whose per-slice G and left are in the fixture (M <= 16)


@functools.lru_cache(maxsize=None)
def golden():
    return dict(numpy.load(os.path.join(HERE, "golden", "thermal_hubbard_cont.npz")))


def system_and_trial(pre):
    from pauxy_amd.systems import Hubbard
    from pauxy_amd.trial_density import OneBody
    d = golden()
    ne = int(d[pre + 'nelec'])
    system = Hubbard(int(d[pre + 'nx']), int(d[pre + 'ny']), ne, ne, float(d[pre + 'U']), mu=float(d[pre + 'mu_system']))
    trial = OneBody(system, float(d[pre + 'beta']), float(d[pre + 'dt']))
    return system, trial


class Qmc(object):
    def __init__(self, dt, nwalkers=1, nstblz=10):
        self.dt, self.nstblz = dt, nstblz
        self.nwalkers = self.ntot_walkers = nwalkers


def ref_path(pre, kit, nw=1, stack_size=None):
    """The restatement's Path of a fixture case on the fixture's own constants (the fp64 numbers the device gets)."""
    d = golden()
    system, _ = system_and_trial(pre)
    L = int(round(float(d[pre + 'beta']) / float(d[pre + 'dt'])))
    ss = int(d[pre + 'stack_size']) if stack_size is None else stack_size
    return R.Path(system.H1, float(d[pre + 'U']), d[pre + 'dmat'], d[pre + 'dmat_inv'], d[pre + 'BH1'], d[pre + 'mf_shift'],
                  complex(d[pre + 'mf_const_fac']), float(d[pre + 'dt']), L, ss, nw, kit=kit)


@functools.lru_cache(maxsize=None)
def ref_run(k, ext):
    """Case a<k> slice by slice through the restatement (ext: numpy.clongdouble) -> dict of per-slice xbar, cmf, cfb,
    G, M0, weight, bin (the bin the slice wrote), and G0, M00, energy, nav, nclip, nkill."""
    d = golden()
    pre = 'a%d_' % k
    p = ref_path(pre, KitExt if ext else Kit64)
    out = {n: [] for n in ('xbar', 'cmf', 'cfb', 'G', 'M0', 'weight', 'bin')}
    out['G0'], out['M00'] = p.G[0].copy(), p.M0[0].copy()
    for ts in range(p.L):
        block = p.block
        xbar, cmf, cfb = p.step(d[pre + 'xi'][ts][None])
        out['xbar'].append(xbar[0]); out['cmf'].append(cmf[0]); out['cfb'].append(cfb[0])
        out['G'].append(p.G[0].copy()); out['M0'].append(p.M0[0].copy()); out['weight'].append(p.weight[0])
        out['bin'].append(p.stack[0, block].copy())
    E, nav = p.energy()
    out.update(energy=E[0], nav=nav[0], nclip=p.nclip, nkill=p.nkill, min_cos_margin=p.min_cos_margin)
    return {n: numpy.array(v) if isinstance(v, list) else v for n, v in out.items()}


def driver_fields(pre):
    """(xis [2 L, nw, M], rs) of a driver run: the stream of its seed, as the fixture's generator replayed it."""
    d = golden()
    nw, L, M = int(d[pre + 'nwalkers']), int(d[pre + 'ntime_slices']), int(d[pre + 'nx']) * int(d[pre + 'ny'])
    npop = int(d[pre + 'npop_control'])
    rs = numpy.random.RandomState(int(d[pre + 'seed']))
    xis, us = [], []
    for _ in range(2):
        for ts in range(L):
            xis.append(rs.normal(0.0, 1.0, (nw, M)))
            if ts % npop == 0 and ts != 0:
                us.append(rs.random_sample())
    return numpy.array(xis), numpy.array(us)


@functools.lru_cache(maxsize=None)
def ref_driver(k, ext):
    """Driver run b<k> through the restatement -> (rows [3, 10], weights [2 L, nw], parents, path)."""
    d = golden()
    pre = 'b%d_' % k
    system, trial = system_and_trial(pre)
    dt = float(d[pre + 'dt'])
    BH1, mf_shift, _, mfc = R.constants(system.T[0], system.U, system.mu, dt, numpy.asarray(trial.dmat.real))
    xis, us = driver_fields(pre)
    p = R.Path(system.H1, system.U, trial.dmat.real, trial.dmat_inv.real, BH1, mf_shift, mfc, dt, int(d[pre + 'ntime_slices']),
               int(d[pre + 'stack_size']), int(d[pre + 'nwalkers']), kit=KitExt if ext else Kit64)
    rows, wts, parents = p.run(xis, us, 2, int(d[pre + 'npop_control']))
    return rows, wts, parents, p


# ---- the device
def device_of(system, BT, BT_inv, BH1, mf_shift, mf_const_fac, dt, L, stack_size, nw, options=0):
    """A handle configured by afq_thermal_configure_hubbard_continuous."""
    from pauxy_amd.device import AfqDevice
    dev = AfqDevice(0)
    try:
        dev.set_system_hubbard(numpy.asarray(system.H1).astype(complex), system.U, system.nup, system.ndown)
        dev.walkers_alloc(nw)
        dev.thermal_configure_hubbard_continuous(L, stack_size, dt, BT, BT_inv, BH1, mf_shift, mf_const_fac, options)
    except Exception:
        dev.close()
        raise
    return dev


def device(pre, nw, stack_size=None, options=0):
    """The device on a fixture case's own constants (what ref_path runs on)."""
    d = golden()
    system, _ = system_and_trial(pre)
    L = int(round(float(d[pre + 'beta']) / float(d[pre + 'dt'])))
    ss = int(d[pre + 'stack_size']) if stack_size is None else stack_size
    return device_of(system, d[pre + 'dmat'], d[pre + 'dmat_inv'], d[pre + 'BH1'], d[pre + 'mf_shift'],
                     complex(d[pre + 'mf_const_fac']), float(d[pre + 'dt']), L, ss, nw, options)


class Chain(object):
    """A 1-D Hubbard chain of M sites (how the kernels' bounds on M are hit exactly), its trial and the constants of
    the restatement; paths of L slices."""

    def __init__(self, M, U=4.0, mu=1.0, dt=0.05, L=4):
        from pauxy_amd.systems import Hubbard
        from pauxy_amd.trial_density import OneBody
        ne = max(1, (M * 7) // 16)
        self.system = Hubbard(M, 1, ne, ne, U, mu=mu)
        self.trial = OneBody(self.system, L * dt, dt)
        self.M, self.dt, self.L = M, dt, L
        self.BT, self.BT_inv = numpy.asarray(self.trial.dmat.real), numpy.asarray(self.trial.dmat_inv.real)
        self.BH1, self.mf_shift, _, self.mfc = R.constants(self.system.T[0], U, mu, dt, self.BT)

    def path(self, stack_size, nw, ext):
        return R.Path(self.system.H1, self.system.U, self.BT, self.BT_inv, self.BH1, self.mf_shift, self.mfc, self.dt,
                      self.L, stack_size, nw, kit=KitExt if ext else Kit64)

    def device(self, stack_size, nw, options=0):
        return device_of(self.system, self.BT, self.BT_inv, self.BH1, self.mf_shift, self.mfc, self.dt, self.L,
                         stack_size, nw, options)
