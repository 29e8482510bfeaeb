#!/usr/bin/env python3
"""Milliseconds per imaginary-time Green's function window (afq_itcf_update, k_itcf.hip) at C3 sizes (M = 100,
K = 500, 25+25, 256 walkers, nmax = 20) and for the discrete-field 4x4 Hubbard model (7+7, 256 walkers, nmax = 20);
model flops of the batched GEMMs and their fraction of the 78.6 TF/s fp64 MFMA peak (the Gauss-Jordan inverses are
counted apart).  One JSON line.  The times are host wall clock around afq_itcf_update, which includes the backward pass
and the copy of the [nmax + 1, 2, 2, M, M] sums to the host; the scratch is kept on the handle after the first window.

  python tools/itcf_bench.py [--reps 3] [--nmax 20]
"""
import argparse
import json
import os
import sys
import time

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pauxy_amd import _lib as L                       # noqa: E402
from tests.helpers import make_device                 # noqa: E402
from tests.itcf_models import generic_model, hirsch_device      # noqa: E402

PEAK = 78.6e12


def gemm_flops(M, nw, nmax, generic):
    """MFMA GEMM work: complex M^3 multiply-adds at 8 flops per (walker, slice).  Generic: 5 Taylor products + 8 for
    BT2 E BT2 and its inverse (two per spin each) + 8 for the chains (two per spin and function); Hubbard: 4 + 8."""
    per = (5 + 8 + 8) if generic else (4 + 8)
    return 8.0 * per * M ** 3 * nw * nmax


def gj_flops(M, nw, nmax):
    """The Gauss-Jordan inverse of E per (walker, slice), 8 M^3 on the vector units (Generic only)."""
    return 8.0 * M ** 3 * nw * nmax


def time_windows(dev, step, psi, nmax, reps):
    out = []
    for _ in range(reps + 1):
        for _ in range(nmax):
            step()
        dev.sync()
        t0 = time.perf_counter()
        dev.itcf_update(psi, 5)
        out.append(time.perf_counter() - t0)
    return out[1:]                                      # the first window pays the first-launch costs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--nmax', type=int, default=20)
    ap.add_argument('--walkers', type=int, default=256)
    args = ap.parse_args()
    nw, nmax = args.walkers, args.nmax
    res = {}
    M, K, na, nb = 100, 500, 25, 25
    model, s, rng = generic_model(M, K, na, nb)
    dev = make_device(model, nw)
    ne = na + nb
    dev.set(L.F_PHI, numpy.array([model.psi + 0.05 * rng.rand(M, ne) for _ in range(nw)]))
    dev.set(L.F_OT, dev.calc_overlap())
    dev.itcf_configure(nmax, 0, True, False)
    t = time_windows(dev, lambda: dev.propagate(rng.normal(size=(nw, K)), 0.2), model.psi, nmax, args.reps)
    fl = gemm_flops(M, nw, nmax, True)
    res['c3'] = {'M': M, 'K': K, 'nelec': [na, nb], 'walkers': nw, 'nmax': nmax, 'ms_per_window': 1e3 * min(t),
                 'gemm_flop': fl, 'gemm_frac_fp64_peak': fl / min(t) / PEAK, 'gj_flop': gj_flops(M, nw, nmax)}
    dev.close()
    dev, BT2, psi, rng, U, dt = hirsch_device(4, 4, 7, 7, nw)
    dev.itcf_configure(nmax, 0, True, False)

    def hstep():
        dev.hirsch_kinetic()
        dev.hirsch_two_body(rng.random_sample((nw, 16)))
        dev.hirsch_finish(0.0)
    t = time_windows(dev, hstep, psi, nmax, args.reps)
    fl = gemm_flops(16, nw, nmax, False)
    res['hubbard_4x4'] = {'M': 16, 'nelec': [7, 7], 'walkers': nw, 'nmax': nmax, 'ms_per_window': 1e3 * min(t),
                          'gemm_flop': fl, 'gemm_frac_fp64_peak': fl / min(t) / PEAK}
    dev.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
