#!/usr/bin/env python3
"""Cost of the finite-temperature UEG path with continuous fields (k_thermal_cplx.hip) per time slice: rs = 1, ecut = 2
(M = 33 plane waves, 512 fields), 2 + 2 electrons, mu = 0.245, beta = 1 in 20 slices of dt = 0.05, OneBody trial, stack_size
5 (4 bins), 256 walkers.  Prints one JSON line (and writes it to --out).

The kernels are timed with event pairs around every launch (afq_launch_trace) over `--paths` whole paths after
`--warmup` paths; the fields come from the host (numpy), as in a run.  Per kernel: launches, total and mean ms.
  thermal_crdm_kernel      P = I - G^T of every walker
  vbias_ueg_lds_kernel     the plane-wave force bias of P (k_models.hip); vbias_ueg_kernel where P does not fit its LDS
                           (M = 123): one of the two has no launches
  thermal_cfields_kernel   clip, shifted fields, cmf, cfb
  vhs_ueg_kernel           the plane-wave HS potential (k_models.hip)
  thermal_cslice_kernel    BV by five Horner products, B, right <- B right, the bin
  thermal_cgreens_kernel   the complex stratified G of all bins and det G (every slice, and once per reset);
                           with --streamed thermal_cgreens_streamed_kernel, T in device memory (needed above M = 47);
                           with --wide thermal_cgreens_wide_kernel and thermal_cslice_wide_kernel, one matrix in LDS
                           (AFQ_THERMAL_WIDE, needed above M = 57: ecut 3.0 is M = 81, ecut 4.0 is M = 93);
                           with --far thermal_cgreens_far_kernel and thermal_cslice_far_kernel, no matrix in LDS
                           (AFQ_THERMAL_FAR, needed above M = 95: ecut 4.5 is M = 123);
                           with --quad thermal_cgreens_quad_kernel and thermal_cslice_quad_kernel, four columns per lane
                           (AFQ_THERMAL_QUAD, needed above M = 128: ecut 5.0 is M = 147)
  thermal_cweight_kernel   the phaseless weight update
`slice_ms` = all of them over the slices run; `path_wall_ms` the host's wall time of a path, fields and copies included
(median and spread over the paths), taken in a separate pass without the event pairs.

With `--alternate N` the resident and the streamed engine are run in turn, N times each, on the same shape (M <= 47):
the JSON then holds every run's figures under `runs` and the median and spread of slice_ms, of the Green's kernel's
mean and of the path's wall time per engine.  `--alternate N --wide` sets the streamed and the wide route side by side
instead (M <= 57), `--alternate N --far` the wide and the far route (M <= 95), `--alternate N --quad` the far and the
quad route (M <= 128).

  python tools/thermal_ueg_bench.py [--paths 5] [--warmup 2] [--ecut 2.0] [--stack-size 5]
                                    [--streamed | --wide | --far | --quad | --alternate N [--wide | --far | --quad]] [--out FILE]
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
from pauxy_amd.propagation.thermal_planewave import planewave_constants        # noqa: E402
from pauxy_amd.systems import UEG                                               # noqa: E402
from pauxy_amd.trial_density import OneBody                                     # noqa: E402

GREENS = {'resident': 'thermal_cgreens_kernel', 'streamed': 'thermal_cgreens_streamed_kernel',
          'wide': 'thermal_cgreens_wide_kernel', 'far': 'thermal_cgreens_far_kernel', 'quad': 'thermal_cgreens_quad_kernel'}
SLICE = {'resident': 'thermal_cslice_kernel', 'streamed': 'thermal_cslice_kernel', 'wide': 'thermal_cslice_wide_kernel',
         'far': 'thermal_cslice_far_kernel', 'quad': 'thermal_cslice_quad_kernel'}
OPTIONS = {'resident': 0, 'streamed': L.THERMAL_STREAMED_GREENS, 'wide': L.THERMAL_WIDE, 'far': L.THERMAL_FAR,
           'quad': L.THERMAL_QUAD}


def kernels_of(engine):
    return ('thermal_crdm_kernel', 'vbias_ueg_lds_kernel', 'vbias_ueg_kernel', 'thermal_cfields_kernel', 'vhs_ueg_kernel',
            SLICE[engine], GREENS[engine],
            'thermal_cweight_kernel')


def one_path(dev, rng, nslices, M00):
    dev.thermal_reset()
    dev.set(L.F_THERMAL_M0, M00)
    for _ in range(nslices):
        dev.thermal_propagate_continuous(rng.normal(size=(dev.nw, dev.K)))
    dev.sync()


def spread(values):
    return {'median': float(numpy.median(values)), 'min': float(min(values)), 'max': float(max(values))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ecut', type=float, default=2.0)
    ap.add_argument('--walkers', type=int, default=256)
    ap.add_argument('--beta', type=float, default=1.0)
    ap.add_argument('--dt', type=float, default=0.05)
    ap.add_argument('--stack-size', type=int, default=5)
    ap.add_argument('--paths', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--streamed', action='store_true', help='AFQ_THERMAL_STREAMED_GREENS: T of the Green\'s function in device memory')
    ap.add_argument('--wide', action='store_true', help='AFQ_THERMAL_WIDE: one matrix in LDS, two columns per lane')
    ap.add_argument('--far', action='store_true', help='AFQ_THERMAL_FAR: no matrix in LDS, two columns per lane')
    ap.add_argument('--quad', action='store_true', help='AFQ_THERMAL_QUAD: no matrix in LDS, four columns per lane')
    ap.add_argument('--alternate', type=int, default=0, help='N runs each of the resident and the streamed engine, in turn '
                    '(with --wide: of the streamed and the wide route; with --far: of the wide and the far route; with --quad: of the '
                    'far and the quad route)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.alternate > 0:
        base, other = ('far', 'quad') if a.quad else ('wide', 'far') if a.far else ('streamed', 'wide') if a.wide else ('resident', 'streamed')
        runs = {base: [], other: []}
        for _ in range(a.alternate):
            for name in (base, other):
                runs[name].append(run(a, name))
        res = dict((k, v) for k, v in runs[base][0].items() if k not in ('kernels', 'slice_ms', 'path_wall_ms', 'finite', 'engine'))
        res['rounds'] = a.alternate
        for name in (base, other):
            g = GREENS[name]
            res[name] = {'slice_ms': spread([r['slice_ms'] for r in runs[name]]),
                         'greens_mean_ms': spread([r['kernels'][g]['mean_ms'] for r in runs[name]]),
                         'slice_kernel_mean_ms': spread([r['kernels'][SLICE[name]]['mean_ms'] for r in runs[name]]),
                         'path_wall_ms': spread([r['path_wall_ms']['median'] for r in runs[name]]),
                         'finite': all(r['finite'] for r in runs[name])}
        res['%s_over_%s' % (other, base)] = {k: res[other][k]['median'] / res[base][k]['median']
                                             for k in ('slice_ms', 'greens_mean_ms', 'slice_kernel_mean_ms', 'path_wall_ms')}
        res['runs'] = runs
    else:
        res = run(a, 'quad' if a.quad else 'far' if a.far else 'wide' if a.wide else 'streamed' if a.streamed else 'resident')
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + "\n")


def run(a, engine):
    s = UEG(1.0, 2, 2, a.ecut, full_lists=True, mu=0.245)
    trial = OneBody(s, a.beta, a.dt)
    nslices = trial.num_slices
    BH1, mf_shift = planewave_constants(s, trial, a.dt)
    dev = AfqDevice(0)
    dev.set_system_ueg(s.iA, s.iB, s.ikpq_i, s.ikpq_kpq, s.ipmq_i, s.ipmq_pmq, s.vqvec, s.vol,
                       numpy.array([s.H1[0].diagonal(), s.H1[1].diagonal()]), s.ecore, s.nup, s.ndown)
    dev.walkers_alloc(a.walkers)
    dev.thermal_configure_continuous(nslices, a.stack_size, a.dt, trial.dmat, trial.dmat_inv, BH1, mf_shift,
                                     options=OPTIONS[engine])
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
    res = {'system': 'UEG rs=1 ecut=%g 2+2 mu=0.245' % a.ecut, 'M': s.nbasis, 'fields': s.nfields, 'walkers': a.walkers,
           'beta': a.beta, 'dt': a.dt, 'slices': nslices, 'stack_size': a.stack_size, 'nbins': nslices // a.stack_size,
           'trial_mu': trial.mu, 'paths': a.paths, 'engine': engine, 'kernels': {}}
    total = 0.0
    for k in kernels_of(engine):
        n, ms = trace.get(k, (0, 0.0))
        res['kernels'][k] = {'launches': n, 'total_ms': ms, 'mean_ms': ms / n if n else 0.0}
        total += ms
    res['slice_ms'] = total / (a.paths * nslices)
    res['path_wall_ms'] = {'median': float(numpy.median(wall)), 'min': float(min(wall)), 'max': float(max(wall))}
    E, nav = dev.thermal_energy()
    res['finite'] = bool(numpy.all(numpy.isfinite(E)) and numpy.all(numpy.isfinite(nav)))
    dev.close()
    return res


if __name__ == '__main__':
    main()
