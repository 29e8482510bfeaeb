#!/usr/bin/env python3
"""Cost of the finite-temperature Hubbard path with continuous fields (k_thermal_cplx.hip, the dense-trial kernels) per
time slice: Hubbard 6 x 6, U = 4, mu = 1, 17 + 17 electrons, beta = 1 in 20 slices of dt = 0.05, OneBody trial,
stack_size 5 (4 bins), 256 walkers.  The resident and the streamed Green's function are run in turn, `--rounds` times
each; the JSON holds every run's figures under `runs` and per engine the median and min - max of the figures below.
Prints one JSON line (and writes it to --out).

The kernels are timed with event pairs around every launch (afq_launch_trace) over `--paths` whole paths after
`--warmup` paths; the fields come from the host (numpy), as in a run.  Per kernel: launches, total and mean ms.
  thermal_crdm_kernel            P = I - G^T of every walker
  thermal_cfields_dense_kernel   force bias from P's diagonal, clip, shifted fields, cmf, cfb, the diagonal of BV
  thermal_cslice_dense_kernel    B = BH1 (BV BH1), right <- B right, bin = left_k right
  thermal_cgreens_kernel         the complex stratified G of all bins and det G (every slice, and once per reset);
                                 streamed: thermal_cgreens_streamed_kernel, T in device memory
  thermal_cweight_mf_kernel      the phaseless weight update with mf_const_fac
With `--wide` the engines run in turn are the wide route alone (AFQ_THERMAL_WIDE: thermal_cgreens_wide_kernel and
thermal_cslice_dense_wide_kernel, one matrix in LDS), which is the only one above 63 sites (`--nx 8`).
With `--far` the far route (AFQ_THERMAL_FAR: thermal_cgreens_far_kernel and thermal_cslice_dense_far_kernel, no matrix
in LDS) runs in turn with the wide route to 95 sites and alone above (`--nx 8 --ny 16`: M = 128).
With `--quad` the quad route (AFQ_THERMAL_QUAD: thermal_cgreens_quad_kernel and thermal_cslice_dense_quad_kernel, four
columns per lane) runs in turn with the far route to 128 sites and alone above (`--nx 12`: M = 144; `--nx 16`: M = 256).
`slice_ms` = all of them over the slices run; `path_kernel_ms` = the same per path; `path_wall_ms` the host's wall time
of a path, fields and copies included, taken in a separate pass without the event pairs.

  python tools/thermal_hubbard_cont_bench.py [--rounds 3] [--paths 5] [--warmup 2] [--nx 6] [--ny NX] [--stack-size 5] [--wide | --far | --quad] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pauxy_amd import _lib as L                                                 # noqa: E402
from pauxy_amd.device import AfqDevice                                          # noqa: E402
from pauxy_amd.propagation.thermal_continuous import Continuous                # noqa: E402
from pauxy_amd.systems import Hubbard                                           # noqa: E402
from pauxy_amd.trial_density import OneBody                                     # noqa: E402

GREENS = {'resident': 'thermal_cgreens_kernel', 'streamed': 'thermal_cgreens_streamed_kernel',
          'wide': 'thermal_cgreens_wide_kernel', 'far': 'thermal_cgreens_far_kernel', 'quad': 'thermal_cgreens_quad_kernel'}
OPTIONS = {'resident': 0, 'streamed': L.THERMAL_STREAMED_GREENS, 'wide': L.THERMAL_WIDE, 'far': L.THERMAL_FAR,
           'quad': L.THERMAL_QUAD}
SMALL = ('thermal_crdm_kernel', 'thermal_cfields_dense_kernel', 'thermal_cweight_mf_kernel')


def slice_of(engine):
    return {'wide': 'thermal_cslice_dense_wide_kernel', 'far': 'thermal_cslice_dense_far_kernel',
            'quad': 'thermal_cslice_dense_quad_kernel'}.get(engine, 'thermal_cslice_dense_kernel')


class Qmc(object):
    def __init__(self, dt):
        self.dt, self.nstblz = dt, 1


def one_path(dev, rng, nslices, M00):
    dev.thermal_reset()
    dev.set(L.F_THERMAL_M0, M00)
    for _ in range(nslices):
        dev.thermal_propagate_continuous(rng.normal(size=(dev.nw, dev.K)))
    dev.sync()


def spread(values):
    return {'median': float(numpy.median(values)), 'min': float(min(values)), 'max': float(max(values))}


def run(a, engine):
    M = a.nx * a.ny
    system = Hubbard(a.nx, a.ny, M // 2 - 1, M // 2 - 1, 4.0, mu=1.0)
    trial = OneBody(system, a.beta, a.dt)
    nslices = trial.num_slices
    prop = Continuous({}, Qmc(a.dt), system, trial)
    dev = AfqDevice(0)
    dev.set_system_hubbard(numpy.asarray(system.T, dtype=complex), system.U, system.nup, system.ndown)
    dev.walkers_alloc(a.walkers)
    dev.thermal_configure_hubbard_continuous(nslices, a.stack_size, a.dt, trial.dmat, trial.dmat_inv, prop.BH1,
                                             prop.mf_shift, prop.mf_const_fac,
                                             OPTIONS[engine])
    M00 = dev.get(L.F_THERMAL_M0)
    rng = numpy.random.RandomState(5)
    for _ in range(a.warmup):
        one_path(dev, rng, nslices, M00)
    wall = []
    for _ in range(a.paths):
        t0 = time.perf_counter()
        one_path(dev, rng, nslices, M00)
        wall.append((time.perf_counter() - t0) * 1e3)
    dev.launch_trace(True)
    for _ in range(a.paths):
        one_path(dev, rng, nslices, M00)
    trace = dev.launch_trace_get()
    dev.launch_trace(False)
    res = {'system': 'Hubbard %dx%d U=4 mu=1' % (a.nx, a.ny), 'M': M, 'walkers': a.walkers, 'beta': a.beta, 'dt': a.dt,
           'slices': nslices, 'stack_size': a.stack_size, 'nbins': nslices // a.stack_size, 'trial_mu': trial.mu,
           'paths': a.paths, 'engine': engine, 'kernels': {}}
    total = 0.0
    for k in SMALL + (slice_of(engine), GREENS[engine]):
        n, ms = trace.get(k, (0, 0.0))
        res['kernels'][k] = {'launches': n, 'total_ms': ms, 'mean_ms': ms / n if n else 0.0}
        total += ms
    res['slice_ms'] = total / (a.paths * nslices)
    res['path_kernel_ms'] = total / a.paths
    res['small_kernels_mean_ms'] = sum(res['kernels'][k]['mean_ms'] for k in SMALL)
    res['path_wall_ms'] = spread(wall)
    E, nav = dev.thermal_energy()
    res['finite'] = bool(numpy.all(numpy.isfinite(E)) and numpy.all(numpy.isfinite(nav)))
    dev.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=6)
    ap.add_argument('--ny', type=int, default=0, help='0: a square lattice, nx x nx')
    ap.add_argument('--walkers', type=int, default=256)
    ap.add_argument('--beta', type=float, default=1.0)
    ap.add_argument('--dt', type=float, default=0.05)
    ap.add_argument('--stack-size', type=int, default=5)
    ap.add_argument('--paths', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3, help='runs of each engine, resident and streamed in turn')
    ap.add_argument('--wide', action='store_true', help='the wide route alone (AFQ_THERMAL_WIDE); with --nx 6 beside the other two')
    ap.add_argument('--far', action='store_true', help='the far route (AFQ_THERMAL_FAR), beside the wide route to 95 sites')
    ap.add_argument('--quad', action='store_true', help='the quad route (AFQ_THERMAL_QUAD), beside the far route to 128 sites')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    a.ny = a.ny or a.nx
    if a.quad:
        names = ('far', 'quad') if a.nx * a.ny <= 128 else ('quad',)
    elif a.far:
        names = ('wide', 'far') if a.nx * a.ny <= 95 else ('far',)
    else:
        names = (('resident', 'streamed', 'wide') if a.nx * a.ny <= 47 else ('wide',)) if a.wide else ('resident', 'streamed')
    runs = {name: [] for name in names}
    for _ in range(a.rounds):
        for name in names:
            runs[name].append(run(a, name))
    res = dict((k, v) for k, v in runs[names[0]][0].items()
               if k not in ('kernels', 'slice_ms', 'path_kernel_ms', 'small_kernels_mean_ms', 'path_wall_ms', 'finite', 'engine'))
    res['rounds'] = a.rounds
    for name in names:
        g = GREENS[name]
        res[name] = {'slice_kernel_mean_ms': spread([r['kernels'][slice_of(name)]['mean_ms'] for r in runs[name]]),
                     'greens_mean_ms': spread([r['kernels'][g]['mean_ms'] for r in runs[name]]),
                     'small_kernels_mean_ms': spread([r['small_kernels_mean_ms'] for r in runs[name]]),
                     'slice_ms': spread([r['slice_ms'] for r in runs[name]]),
                     'path_kernel_ms': spread([r['path_kernel_ms'] for r in runs[name]]),
                     'path_wall_ms': spread([r['path_wall_ms']['median'] for r in runs[name]]),
                     'finite': all(r['finite'] for r in runs[name])}
    for other, base in (('streamed', 'resident'), ('wide', 'streamed'), ('far', 'wide'), ('quad', 'far')):
        if other in res and base in res:
            res['%s_over_%s' % (other, base)] = {k: res[other][k]['median'] / res[base][k]['median']
                                                 for k in ('slice_ms', 'greens_mean_ms', 'path_wall_ms') +
                                                 (('slice_kernel_mean_ms',) if other in ('far', 'quad') else ())}
    res['runs'] = runs
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == '__main__':
    main()
