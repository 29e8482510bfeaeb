"""What the CPU and the GPU tests of the wide route (AFQ_THERMAL_WIDE) share: the three fixtures recorded from the
reference (tests/golden/thermal_ueg81.npz, thermal_ueg93.npz, thermal_hubbard_cont_wide.npz), the restatements
(tests/thermal_ueg_ref.py, tests/thermal_hubbard_cont_ref.py) run over a fixture case in either kit, and their stored
extended-precision results (tests/golden/thermal_ueg81_ext.npz, thermal_ueg93_ext.npz,
thermal_hubbard_cont_wide_ext.npz, written by tests/golden/make_thermal_wide_ext.py: the numpy.clongdouble restatement
of a slice at M = 93 takes seconds, of a driver run minutes).

Stored extended numbers are the sum of two parts, <key>_hi (float64 / complex128) and <key>_lo (the remainder; the
Green's functions keep it as complex64, which places them to 1e-24 of their scale)."""
import functools
import os

import numpy

from tests import thermal_hubbard_cont_ref as R
from tests.thermal_ueg_cases import Case
from tests.thermal_ueg_ref import Kit64
from tests.thermal_ueg_ref_ext import KitExt

HERE = os.path.dirname(os.path.abspath(__file__))
ECUT_OF_M = {7: 0.5, 19: 1.0, 27: 1.5, 33: 2.0, 57: 2.5, 81: 3.0, 93: 4.0}
UEG_A = (("thermal_ueg81.npz", "a6_"), ("thermal_ueg93.npz", "a7_"))      # the single-walker cases
UEG_B = ("thermal_ueg81.npz", 5)                                          # the driver run b5
HUBBARD = "thermal_hubbard_cont_wide.npz"
HUBBARD_A, HUBBARD_B = (8, 9), 2
EXT_OF = {"thermal_ueg81.npz": "thermal_ueg81_ext.npz", "thermal_ueg93.npz": "thermal_ueg93_ext.npz",
          HUBBARD: "thermal_hubbard_cont_wide_ext.npz"}
SCALARS = ('xbar', 'cmf', 'cfb', 'M0', 'weight')


@functools.lru_cache(maxsize=None)
def golden(name):
    return dict(numpy.load(os.path.join(HERE, "golden", name)))


def stored_ext():
    """Every stored extended result, of the three files, by key."""
    out = {}
    for name in EXT_OF.values():
        out.update(golden(name))
    return out


def split(x, small=False):
    """An extended array as (hi, lo) with hi + lo == x to the last bit (small: lo in single precision)."""
    x = numpy.asarray(x)
    cx = numpy.iscomplexobj(x)
    hi = x.astype(numpy.complex128 if cx else numpy.float64)
    lo = (x - hi).astype((numpy.complex64 if small else numpy.complex128) if cx else (numpy.float32 if small else numpy.float64))
    return hi, lo


def joined(x, key):
    hi, lo = x[key + '_hi'], x[key + '_lo']
    t = numpy.clongdouble if numpy.iscomplexobj(hi) else numpy.longdouble
    return numpy.asarray(hi, dtype=t) + numpy.asarray(lo, dtype=t)


_UEG = {}


def ueg_case(M):
    """One Case per basis size for a process (the operators are built once)."""
    if M not in _UEG:
        _UEG[M] = Case(ECUT_OF_M[M], 2 if M > 7 else 1)
    return _UEG[M]


def case_of_fixture(d, pre):
    return Case(float(d[pre + 'ecut']), int(d[pre + 'nelec']), rs=float(d[pre + 'rs']), beta=float(d[pre + 'beta']),
                dt=float(d[pre + 'dt']), mu=float(d[pre + 'mu_system']), fb_bound=float(d[pre + 'fb_bound']))


def ueg_run(name, pre, ext, nslice=None):
    """A single-walker UEG case slice by slice through the restatement -> dict of per-slice xbar, cmf, cfb, M0, weight,
    G at the fixture's G_slices, and M00, energy, nav, nclip, min_cos_margin."""
    d = golden(name)
    c = case_of_fixture(d, pre)
    ss = int(d[pre + 'stack_size'])
    p = c.path_ext(ss, 1) if ext else c.path64(ss, 1)
    keep = set(int(n) for n in d[pre + 'G_slices'])
    out = {n: [] for n in SCALARS + ('G',)}
    out['M00'] = p.M0[0].copy()
    for ts in range(c.L if nslice is None else nslice):
        xbar, cmf, cfb = p.step(d[pre + 'xi'][ts][None])
        out['xbar'].append(xbar[0]); out['cmf'].append(cmf[0]); out['cfb'].append(cfb[0])
        out['M0'].append(p.M0[0].copy()); out['weight'].append(p.weight[0])
        if ts + 1 in keep:
            out['G'].append(p.G[0].copy())
    E, nav = p.energy()
    out.update(energy=E[0], nav=nav[0], nclip=p.nclip, min_cos_margin=p.min_cos_margin)
    return {n: numpy.array(v) if isinstance(v, list) else v for n, v in out.items()}


# ---- the Hubbard cases
def hubbard_system(d, pre):
    from pauxy_amd.systems import Hubbard
    ne = int(d[pre + 'nelec'])
    return Hubbard(int(d[pre + 'nx']), int(d[pre + 'ny']), ne, ne, float(d[pre + 'U']), mu=float(d[pre + 'mu_system']))


def hubbard_path(d, pre, ext, nw=1):
    """The restatement's Path of a fixture case on the fixture's own constants (the fp64 numbers the device gets)."""
    system = hubbard_system(d, pre)
    L = int(round(float(d[pre + 'beta']) / float(d[pre + 'dt'])))
    return R.Path(system.H1, float(d[pre + 'U']), d[pre + 'dmat'], d[pre + 'dmat_inv'], d[pre + 'BH1'], d[pre + 'mf_shift'],
                  complex(d[pre + 'mf_const_fac']), float(d[pre + 'dt']), L, int(d[pre + 'stack_size']), nw,
                  kit=KitExt if ext else Kit64)


def hubbard_device(d, pre, nw, options):
    from tests.thermal_hubbard_cont_cases import device_of
    L = int(round(float(d[pre + 'beta']) / float(d[pre + 'dt'])))
    return device_of(hubbard_system(d, pre), d[pre + 'dmat'], d[pre + 'dmat_inv'], d[pre + 'BH1'], d[pre + 'mf_shift'],
                     complex(d[pre + 'mf_const_fac']), float(d[pre + 'dt']), L, int(d[pre + 'stack_size']), nw, options)


def hubbard_run(k, ext, nslice=None):
    """Case a<k> of the Hubbard fixture slice by slice through the restatement, as ueg_run; G behind the last slice."""
    d = golden(HUBBARD)
    pre = 'a%d_' % k
    p = hubbard_path(d, pre, ext)
    out = {n: [] for n in SCALARS}
    out['M00'] = p.M0[0].copy()
    for ts in range(p.L if nslice is None else nslice):
        xbar, cmf, cfb = p.step(d[pre + 'xi'][ts][None])
        out['xbar'].append(xbar[0]); out['cmf'].append(cmf[0]); out['cfb'].append(cfb[0])
        out['M0'].append(p.M0[0].copy()); out['weight'].append(p.weight[0])
    E, nav = p.energy()
    out.update(G_last=p.G[0].copy(), energy=E[0], nav=nav[0], nclip=p.nclip, min_cos_margin=p.min_cos_margin)
    return {n: numpy.array(v) if isinstance(v, list) else v for n, v in out.items()}


def hubbard_driver_fields(d, pre):
    """(xis [2 L, nw, M], the comb's uniforms) of the driver run: the stream of its seed."""
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


def hubbard_driver(ext):
    """Driver run b2 through the restatement -> (rows [3, 10], weights [2 L, nw], parents, path)."""
    from pauxy_amd.trial_density import OneBody
    d = golden(HUBBARD)
    pre = 'b%d_' % HUBBARD_B
    system = hubbard_system(d, pre)
    dt = float(d[pre + 'dt'])
    trial = OneBody(system, float(d[pre + 'beta']), dt)
    BH1, mf_shift, _, mfc = R.constants(system.T[0], system.U, system.mu, dt, numpy.asarray(trial.dmat.real))
    xis, us = hubbard_driver_fields(d, pre)
    p = R.Path(system.H1, system.U, trial.dmat.real, trial.dmat_inv.real, BH1, mf_shift, mfc, dt, int(d[pre + 'ntime_slices']),
               int(d[pre + 'stack_size']), int(d[pre + 'nwalkers']), kit=KitExt if ext else Kit64)
    rows, wts, parents = p.run(xis, us, 2, int(d[pre + 'npop_control']))
    return rows, wts, parents, p


def hubbard_driver_options(d, pre, **walkers):
    return {'qmc': {'timestep': float(d[pre + 'dt']), 'beta': float(d[pre + 'beta']),
                    'num_walkers': int(d[pre + 'nwalkers']), 'blocks': 2,
                    'pop_control_freq': int(d[pre + 'npop_control']), 'rng_seed': int(d[pre + 'seed'])},
            'model': {'name': 'Hubbard', 'nx': int(d[pre + 'nx']), 'ny': int(d[pre + 'ny']), 'U': float(d[pre + 'U']),
                      'mu': float(d[pre + 'mu_system']), 'nup': int(d[pre + 'nelec']), 'ndown': int(d[pre + 'nelec'])},
            'trial': {'name': 'one_body'},
            'walkers': dict({'stack_size': int(d[pre + 'stack_size']), 'low_rank': False}, **walkers),
            'propagator': {'hubbard_stratonovich': 'continuous'},
            'estimates': {'mixed': {'verbose': False}}}
