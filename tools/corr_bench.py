#!/usr/bin/env python3
"""Cost of the back-propagated correlation functions (two_rdm: 'correlation', k_corr.hip) at the C4 sizes: Hubbard
16 x 16 at half filling, discrete fields, 256 walkers, per back-propagation window of `--nbp` steps.  Prints one JSON line.

  off     afq_bp_update with no option (the path this leaves unchanged)
  on      afq_bp_update_ext with the correlation functions
  extra   on - off (medians)
Timed from the host around the call, stream synchronised before and after; `--warmup` + `--windows` windows of each
kind, median and the run-to-run spread (min, max).  Every window is preceded by its propagation steps (not timed).
The weighted sum reads every walker's G [2, M, M] twice: bytes = 2 * 16 * 2 * M^2 * (walkers of non-zero weight).

  python tools/corr_bench.py [--windows 10] [--warmup 3] [--nbp 4]
  rocprofv3 --kernel-trace --stats -- python tools/corr_bench.py --profile      only 'on' windows, for a kernel trace
"""
import argparse
import json
import os
import sys
import time

import numpy
import scipy.linalg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pauxy_amd import _lib as L, systems                           # noqa: E402
from pauxy_amd.device import AfqDevice                             # noqa: E402


def make(nx, ny, nw, U=4.0, dt=0.01, seed=4):
    na = nb = nx * ny // 2
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
    dev.set_propagator_hirsch(BT2, dt)
    dev.walkers_alloc(nw)
    dev.set(L.F_PHI, numpy.array([psi + 0.05 * rng.rand(M, na + nb) for _ in range(nw)]))
    dev.set(L.F_OT, dev.calc_overlap())
    return dev, psi, rng


def window(dev, psi, rng, nbp, on):
    for step in range(nbp):
        dev.hirsch_kinetic()
        dev.hirsch_two_body(rng.random_sample((dev.nw, dev.M)))
        dev.hirsch_finish(0.0)
    dev.sync()
    t0 = time.perf_counter()
    dev.bp_update(psi, 5, None, False, reset=True, two_rdm=on)
    dev.sync()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return {'median_ms': float(numpy.median(ts)), 'min_ms': float(min(ts)), 'max_ms': float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=16)
    ap.add_argument('--walkers', type=int, default=256)
    ap.add_argument('--nbp', type=int, default=4)
    ap.add_argument('--windows', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--profile', action='store_true')
    a = ap.parse_args()
    dev, psi, rng = make(a.nx, a.nx, a.walkers)
    dev.bp_configure(a.nbp)
    dev.bp_observables(two_rdm='correlation')
    res = {'system': 'Hubbard %dx%d' % (a.nx, a.nx), 'M': dev.M, 'walkers': a.walkers, 'nbp': a.nbp}
    kinds = [True] if a.profile else [False, True]
    for on in kinds:
        ts = [window(dev, psi, rng, a.nbp, on) for _ in range(a.warmup + a.windows)][a.warmup:]
        res['on' if on else 'off'] = stats(ts)
    alive = int(numpy.count_nonzero(dev.get(L.F_WEIGHT)))
    res['walkers_nonzero'] = alive
    res['wsum_bytes'] = 2 * 16 * 2 * dev.M * dev.M * alive
    if not a.profile:
        res['extra_ms'] = res['on']['median_ms'] - res['off']['median_ms']
    dev.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
