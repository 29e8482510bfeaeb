#!/usr/bin/env python3
"""The four driver runs of thermal_ueg.npz (case b) through the two restatements of the tests, stored so that the GPU
tests can hold whole paths to the accuracy rule without running the extended-precision restatement themselves (M = 33
with 12 walkers over two paths takes it about half a minute).

  thermal_ueg_paths_ext.npz, for k = 0 .. 3 (the cases b0 .. b3, fields and comb uniforms replayed from the seed):
    b<k>_w64, b<k>_r64        weights after every slice (before its cap) [2 L, nw] and the estimator rows [3, 10] of
                              tests/thermal_ueg_ref.py (fp64)
    b<k>_wx_hi / _lo, b<k>_rx_hi / _lo
                              the same of tests/thermal_ueg_ref_ext.py (numpy.longdouble) as the sum of two doubles
    b<k>_parents              the comb's parent multiplicities of the extended run
Needs no reference: it reads thermal_ueg.npz only for the parameters of the cases.  tests/test_thermal_ueg_cpu.py
recomputes case b1 and compares it with what is stored here.

Usage:  python tests/golden/make_thermal_ueg_paths_ext.py            (writes tests/golden/thermal_ueg_paths_ext.npz)
        python tests/golden/make_thermal_ueg_paths_ext.py --check    recompute and compare with the committed file
"""
import os
import sys

import numpy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.thermal_ueg_cases import Case                                  # noqa: E402

NAME = 'thermal_ueg_paths_ext.npz'


def split(x):
    """A longdouble array as (hi, lo) doubles with hi + lo == x to the last bit of a 64-bit mantissa."""
    x = numpy.asarray(x, dtype=numpy.longdouble)
    hi = x.astype(numpy.float64)
    return hi, (x - hi).astype(numpy.float64)


def join(hi, lo):
    return numpy.asarray(hi, dtype=numpy.longdouble) + numpy.asarray(lo, dtype=numpy.longdouble)


def stream(d, pre, K):
    """The fields [2 L, nw, K] and the comb uniforms the driver draws from the case's seed."""
    nw, L, npop = int(d[pre + 'nwalkers']), int(d[pre + 'ntime_slices']), int(d[pre + 'npop_control'])
    rs = numpy.random.RandomState(int(d[pre + 'seed']))
    xis, rr = [], []
    for _ in range(2):
        for ts in range(L):
            xis.append(rs.normal(0.0, 1.0, (nw, K)))
            if ts % npop == 0 and ts != 0:
                rr.append(rs.random_sample())
    return numpy.array(xis), rr


def run_case(d, k, kits=('fp64', 'ext')):
    pre = 'b%d_' % k
    c = Case(float(d[pre + 'ecut']), int(d[pre + 'nelec']), beta=float(d[pre + 'beta']), dt=float(d[pre + 'dt']),
             mu=float(d[pre + 'mu_system']))
    nw, ss, npop = int(d[pre + 'nwalkers']), int(d[pre + 'stack_size']), int(d[pre + 'npop_control'])
    xis, rr = stream(d, pre, c.K)
    out = {}
    if 'fp64' in kits:
        rows, wts, _ = c.path64(ss, nw).run(xis, rr, 2, npop)
        out[pre + 'w64'], out[pre + 'r64'] = numpy.asarray(wts, dtype=numpy.float64), numpy.asarray(rows, dtype=numpy.float64)
    if 'ext' in kits:
        rows, wts, parents = c.path_ext(ss, nw).run(xis, rr, 2, npop)
        out[pre + 'wx_hi'], out[pre + 'wx_lo'] = split(wts)
        out[pre + 'rx_hi'], out[pre + 'rx_lo'] = split(rows)
        out[pre + 'parents'] = numpy.array(parents)
    return out


def make():
    d = numpy.load(os.path.join(HERE, 'thermal_ueg.npz'))
    out = {}
    for k in range(4):
        out.update(run_case(d, k))
    return out


if __name__ == '__main__':
    out = make()
    path = os.path.join(HERE, NAME)
    if '--check' in sys.argv[1:]:
        old = numpy.load(path)
        bad = []
        for key, v in out.items():
            exact = not key.endswith(('w64', 'r64'))           # (the fp64 restatement goes through LAPACK)
            ok = numpy.array_equal(old[key], v) if exact else numpy.allclose(old[key], v, rtol=1e-12, atol=0)
            if not ok:
                bad.append(key)
        print('%s %s' % (NAME, 'reproduces' if not bad else 'DIFFERS: ' + ', '.join(bad)))
        sys.exit(1 if bad else 0)
    numpy.savez_compressed(path, **out)
    print('%s %d bytes' % (NAME, os.path.getsize(path)))
