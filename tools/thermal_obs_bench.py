#!/usr/bin/env python3
"""Cost of the averaged estimators of a thermal population (`average_gf`): the batched sweep of afq_thermal_estimates
against the only way to the same numbers without it, the loop of afq_thermal_greens(ts stack_size) +
afq_thermal_energy per bin (one launch per stage and one host round trip per bin; the same bits).

Shapes, each on the stacks one propagated path leaves (beta = 1 in 20 slices of dt = 0.05, OneBody trial):
  UEG rs = 1, ecut = 2 (M = 33), 2 + 2, mu = 0.245: 4 bins (stack_size 5) and 20 bins (stack_size 1), 256 and 16 walkers
  Hubbard 8 x 8, U = 4, mu = 1, discrete fields:    2 bins (stack_size 10), 256 walkers
With `--far` instead the sweep on the wide body: UEG rs = 1, ecut = 3 (M = 81) on a handle configured with
AFQ_THERMAL_FAR, 4 bins, 16 and 256 walkers.
Per shape `--rounds` alternating runs of the two; a run is the host's wall time of `--reps` calls after `--warmup`,
per call, the copies of the results to the host included (both ways end with one).  Medians and (min - max) over the
rounds; `same_bits` says that the sweep's sums equalled the loop's, added in bin order, on this run.  Measured, not
tuned: there is no target.

  python tools/thermal_obs_bench.py [--rounds 3] [--reps 10] [--warmup 2] [--far] [--out profiles/thermal_observables.json]
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
from pauxy_amd.propagation.thermal_hubbard import thermal_constants            # noqa: E402
from pauxy_amd.propagation.thermal_planewave import planewave_constants        # noqa: E402
from pauxy_amd.systems import UEG, Hubbard                                      # noqa: E402
from pauxy_amd.trial_density import OneBody                                     # noqa: E402

BETA, DT = 1.0, 0.05
SHAPES = [('ueg', 5, 256), ('ueg', 5, 16), ('ueg', 1, 256), ('ueg', 1, 16), ('hubbard', 10, 256)]
FAR_SHAPES = [('ueg_far', 5, 16), ('ueg_far', 5, 256)]


def ueg_device(stack_size, nw, ecut=2.0, options=0):
    s = UEG(1.0, 2, 2, ecut, full_lists=True, mu=0.245)
    trial = OneBody(s, BETA, DT)
    BH1, mf_shift = planewave_constants(s, trial, DT)
    dev = AfqDevice(0)
    dev.set_system_ueg(s.iA, s.iB, s.ikpq_i, s.ikpq_kpq, s.ipmq_i, s.ipmq_pmq, s.vqvec, s.vol,
                       numpy.array([s.H1[0].diagonal(), s.H1[1].diagonal()]), s.ecore, s.nup, s.ndown)
    dev.walkers_alloc(nw)
    dev.thermal_configure_continuous(trial.num_slices, stack_size, DT, trial.dmat, trial.dmat_inv, BH1, mf_shift, options=options)
    rng = numpy.random.RandomState(5)
    for _ in range(trial.num_slices):
        dev.thermal_propagate_continuous(rng.normal(size=(nw, dev.K)))
    return dev, 'UEG rs=1 ecut=%g 2+2 mu=0.245%s' % (ecut, ' far_basis' if options else ''), trial.num_slices


def ueg_far_device(stack_size, nw):
    return ueg_device(stack_size, nw, 3.0, L.THERMAL_FAR)


def hubbard_device(stack_size, nw):
    s = Hubbard(8, 8, 31, 31, 4.0, mu=1.0)
    trial = OneBody(s, BETA, DT)
    _, auxf, _, _, BH1 = thermal_constants(s, trial, DT)
    dev = AfqDevice(0)
    dev.set_system_hubbard(numpy.asarray(s.T, dtype=complex), s.U, s.nup, s.ndown)
    dev.walkers_alloc(nw)
    dev.thermal_configure(trial.num_slices, stack_size, stack_size, trial.dmat, trial.dmat_inv, BH1, auxf)
    rng = numpy.random.RandomState(5)
    for _ in range(trial.num_slices):
        dev.thermal_propagate(rng.random_sample((nw, dev.M)))
    return dev, 'Hubbard 8x8 U=4 mu=1 31+31 discrete fields', trial.num_slices


def loop(dev, nbins, stack_size):
    rows = []
    for ts in range(nbins):
        dev.thermal_greens(ts * stack_size)
        E, nav = dev.thermal_energy()
        rows.append(numpy.concatenate([E, nav[:, None]], axis=1))
    return numpy.array(rows)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def spread(values):
    return {'median': float(numpy.median(values)), 'min': float(min(values)), 'max': float(max(values))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--far', action='store_true', help='the sweep on a far handle at M = 81 instead of the shapes above')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    shapes = []
    makers = {'ueg': ueg_device, 'hubbard': hubbard_device, 'ueg_far': ueg_far_device}
    for kind, stack_size, nw in (FAR_SHAPES if a.far else SHAPES):
        dev, system, nslices = makers[kind](stack_size, nw)
        nbins = nslices // stack_size
        try:
            rows = loop(dev, nbins, stack_size)
            res = dev.thermal_estimates(average_gf=True, per_bin=True)
            sums = numpy.zeros_like(rows[0])
            for r in rows:
                sums = sums + r
            same = bool(numpy.array_equal(res['per_bin'], rows) and numpy.array_equal(res['cols'], sums))
            t_loop, t_sweep = [], []
            for _ in range(a.rounds):
                t_loop.append(timed(lambda: loop(dev, nbins, stack_size), a.reps, a.warmup))
                t_sweep.append(timed(lambda: dev.thermal_estimates(average_gf=True), a.reps, a.warmup))
            dev.launch_trace(True)
            dev.thermal_estimates(average_gf=True)
            trace = dev.launch_trace_get()
            dev.launch_trace(False)
        finally:
            dev.close()
        shapes.append({'system': system, 'M': int(dev.M), 'walkers': nw, 'stack_size': stack_size, 'nbins': nbins,
                       'same_bits': same, 'finite': bool(numpy.all(numpy.isfinite(rows))),
                       'loop_ms': spread(t_loop), 'sweep_ms': spread(t_sweep),
                       'sweep_over_loop': float(numpy.median(t_sweep) / numpy.median(t_loop)),
                       'sweep_kernels_ms': {k: v[1] for k, v in trace.items()}})
    res = {'what': 'afq_thermal_estimates(AVERAGE_GF) against the loop afq_thermal_greens + afq_thermal_energy per bin',
           'beta': BETA, 'dt': DT, 'rounds': a.rounds, 'reps': a.reps, 'warmup': a.warmup, 'shapes': shapes}
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == '__main__':
    main()
