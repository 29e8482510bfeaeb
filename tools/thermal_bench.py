#!/usr/bin/env python3
"""Cost of the finite-temperature Hubbard path (k_thermal.hip) per time slice: Hubbard 8 x 8, U = 4, mu = 1, beta = 2,
dt = 0.05 (40 slices), OneBody trial, 256 walkers.  Prints one JSON line (and writes it to --out).

The three kernels are timed with event pairs around every launch (afq_launch_trace) over `--paths` whole paths after
`--warmup` paths; the uniforms come from the host (numpy), as in a run.  Per kernel: launches, total and mean ms.
  thermal_slice_kernel    the M single-site updates of every walker and its stack update (once per slice)
  thermal_greens_kernel   the stratified G from the stack (every nstblz slices, and once per reset)
  thermal_wrap_kernel     G <- BT G BT^-1 (every slice but the last of a path)
With --delayed the handle is configured with AFQ_THERMAL_DELAYED and the first two are thermal_slice_delayed_kernel and
thermal_greens_wide_kernel; --nx / --ny choose the lattice (ny defaults to nx; beyond 64 sites only with --delayed).
`slice_ms` = all three over the slices run; `path_wall_ms` the host's wall time of a path, uniforms and copies included
(median and spread over the paths).  The event pairs cost a few microseconds per launch: the wall time is taken in a
separate pass without them.

  python tools/thermal_bench.py [--nx 8] [--ny 8] [--delayed] [--paths 5] [--warmup 2] [--stack-size N] [--nstblz N] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pauxy_amd import _lib as L_                                          # noqa: E402
from pauxy_amd.device import AfqDevice                                     # noqa: E402
from pauxy_amd.propagation.thermal_hubbard import thermal_constants       # noqa: E402
from pauxy_amd.systems import Hubbard                                      # noqa: E402
from pauxy_amd.trial_density import OneBody                                # noqa: E402

KERNELS = ('thermal_slice_kernel', 'thermal_greens_kernel', 'thermal_wrap_kernel')
KERNELS_DELAYED = ('thermal_slice_delayed_kernel', 'thermal_greens_wide_kernel', 'thermal_wrap_kernel')


def one_path(dev, rng, L):
    dev.thermal_reset()
    for _ in range(L):
        dev.thermal_propagate(rng.random_sample((dev.nw, dev.M)))
    dev.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=8)
    ap.add_argument('--ny', type=int, default=None)
    ap.add_argument('--delayed', action='store_true')
    ap.add_argument('--walkers', type=int, default=256)
    ap.add_argument('--beta', type=float, default=2.0)
    ap.add_argument('--dt', type=float, default=0.05)
    ap.add_argument('--stack-size', type=int, default=None)
    ap.add_argument('--nstblz', type=int, default=None)
    ap.add_argument('--paths', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    ny = a.ny or a.nx
    M = a.nx * ny
    system = Hubbard(a.nx, ny, M // 2 - 1, M // 2 - 1, 4.0, mu=1.0)
    trial = OneBody(system, a.beta, a.dt)
    opts = {} if a.stack_size is None else {'stack_size': a.stack_size}
    ss = opts.get('stack_size', trial.stack_size)
    nstblz = a.nstblz or ss
    L = trial.num_slices
    _, auxf, _, _, BH1 = thermal_constants(system, trial, a.dt)
    dev = AfqDevice(0)
    dev.set_system_hubbard(numpy.asarray(system.T, dtype=complex), system.U, system.nup, system.ndown)
    dev.walkers_alloc(a.walkers)
    dev.thermal_configure(L, ss, nstblz, trial.dmat, trial.dmat_inv, BH1, auxf,
                          L_.THERMAL_DELAYED if a.delayed else 0)
    rng = numpy.random.RandomState(5)
    for _ in range(a.warmup):
        one_path(dev, rng, L)
    wall = []
    for _ in range(a.paths):
        t0 = time.perf_counter()
        one_path(dev, rng, L)
        wall.append((time.perf_counter() - t0) * 1e3)
    dev.launch_trace(True)
    for _ in range(a.paths):
        one_path(dev, rng, L)
    trace = dev.launch_trace_get()
    dev.launch_trace(False)
    res = {'system': 'Hubbard %dx%d U=4 mu=1' % (a.nx, ny), 'M': M, 'route': 'delayed' if a.delayed else 'direct', 'walkers': a.walkers, 'beta': a.beta, 'dt': a.dt,
           'slices': L, 'stack_size': ss, 'nbins': L // ss, 'nstblz': nstblz, 'trial_mu': trial.mu, 'paths': a.paths,
           'kernels': {}}
    total = 0.0
    for k in (KERNELS_DELAYED if a.delayed else KERNELS):
        n, ms = trace.get(k, (0, 0.0))
        res['kernels'][k] = {'launches': n, 'total_ms': ms, 'mean_ms': ms / n if n else 0.0}
        total += ms
    res['slice_ms'] = total / (a.paths * L)
    res['path_wall_ms'] = {'median': float(numpy.median(wall)), 'min': float(min(wall)), 'max': float(max(wall))}
    E, nav = dev.thermal_energy()
    res['finite'] = bool(numpy.all(numpy.isfinite(E)) and numpy.all(numpy.isfinite(nav)))
    dev.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == '__main__':
    main()
