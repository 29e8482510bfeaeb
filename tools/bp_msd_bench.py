#!/usr/bin/env python3
"""Milliseconds per back-propagation window of a multi-determinant trial (afq_bp_update_msd) at C5 sizes (M = 400,
K = 2000, 50+50, 256 walkers, ndet = 4 distinct complex determinants, a history of 3 steps), next to the
single-determinant window (afq_bp_update, whose kernels this change does not touch) at the same sizes on the same
machine in the same process.  One JSON line.

  window_ms            host wall clock around one window (ends in the copy-out of the sums: synchronised), median of
                       --reps windows after a warm-up window, alternating the two handles
  backward_ms          the backward pass alone, from a separate pass under the launch trace (event pairs around every
                       launch): fields + VHS builder + one-body and Taylor products + re-orthogonalisations
  vhs_ms, products_ms  its parts; the multi-determinant window builds V once per step and multiplies the ndet
                       determinants of a walker as one column-stacked operand
  loop_backward_ms     what the determinant loop over the same V would take: vhs_ms of one determinant's window +
                       ndet x (products + re-orthogonalisations of the single-determinant window)
  four_single_ms       ndet x the single-determinant backward pass (V rebuilt per determinant)

  python tools/bp_msd_bench.py [--reps 7] [--walkers 256] [--ndet 4] [--M 400 --K 2000 --N 50]
"""
import argparse
import json
import os
import sys
import time

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import afqmc_ref as ref                   # noqa: E402
from pauxy_amd import _lib as L, systems, trial as trial_mod   # noqa: E402
from pauxy_amd.device import AfqDevice                # noqa: E402
from pauxy_amd.propagation import setup               # noqa: E402
from tests.helpers import make_device                 # noqa: E402

BACKWARD = {'vhs': ('k_vhs_generic', 'vhs_cplx_launch'),
            'products': ('k_bp_msd_onebody', 'k_bp_msd_taylor', 'onebody_spin', 'k_onebody', 'k_apply_exponential', 'prop_fused_kernel'),
            'reortho': ('reortho', 'k_reortho_big', 'bp_msd_logr_kernel', 'chol', 'qr'),
            'fields': ('bp_fields_kernel',)}


def split(trace):
    out = {k: 0.0 for k in BACKWARD}
    rest = 0.0
    for name, (n, ms) in trace.items():
        for part, subs in BACKWARD.items():
            if any(s in name for s in subs):
                out[part] += float(ms)
                break
        else:
            rest += float(ms)
    out['backward'] = sum(out[k] for k in BACKWARD)
    out['rest_of_window'] = rest
    return out


def traced(dev, fn):
    fn()
    dev.launch_trace(True)
    fn()
    trace = dev.launch_trace_get()
    dev.launch_trace(False)
    return split(trace), {k: [int(v[0]), round(float(v[1]), 4)] for k, v in trace.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--walkers', type=int, default=256)
    ap.add_argument('--ndet', type=int, default=4)
    ap.add_argument('--M', type=int, default=400)
    ap.add_argument('--K', type=int, default=2000)
    ap.add_argument('--N', type=int, default=50)
    ap.add_argument('--nbp', type=int, default=3)
    a = ap.parse_args()
    M, K, N, nw, nd, nbp, dt, nstblz = a.M, a.K, a.N, a.walkers, a.ndet, a.nbp, 0.005, 2
    s = systems.synthetic_generic(M, K, (N, N), seed=7)
    t0 = trial_mod.rhf_trial_generic(s)
    rng = numpy.random.RandomState(3)
    dets = numpy.array([t0.psi + 0.05 * (rng.rand(M, 2 * N) + 1j * rng.rand(M, 2 * N)) for d in range(nd)])
    coeffs = numpy.array([0.8 + 0.1j, 0.3 - 0.2j, 0.2 + 0.05j, -0.1 + 0.15j, 0.1 + 0j, 0.05j][:nd])
    t = trial_mod.MultiDetTrial(s, (coeffs, dets), init=t0.psi)
    BH1, mf = setup.generic_propagator_arrays(s, t, dt)
    H1 = numpy.asarray(s.H1).astype(complex)
    per = M * 2 * N
    msd = AfqDevice(0)
    msd.set_system_generic(s.hs_pot, t._rchol[:per], H1, s.ecore, N, N)
    msd.set_trial_multi(dets, coeffs, t._rchol)
    msd.set_propagator(BH1, mf, dt)
    msd.walkers_alloc(nw)
    t1 = trial_mod.SingleDetTrial(s, dets[0])
    one = make_device(ref.RefModel('generic', M, N, N, t1.psi, BH1, mf, dt, hs_pot=s.hs_pot, rchol=t1._rchol, H1=H1,
                                   ecore=s.ecore), nw)
    phis = t0.psi[None] + 0.05 * (rng.rand(nw, M, 2 * N) + 1j * rng.rand(nw, M, 2 * N))
    for dev in (msd, one):
        dev.set(L.F_PHI, phis)
        dev.set(L.F_OT, dev.calc_overlap())
        dev.bp_configure(nbp)
    for _ in range(nbp):
        xi = rng.normal(size=(nw, K))
        for dev in (msd, one):
            dev.propagate(xi, 0.1)
    assert list(msd.bp_steps()) == [nbp] * nw and list(one.bp_steps()) == [nbp] * nw
    f_msd = lambda: msd.bp_update_msd(dets, coeffs, nstblz, None, False, reset=False)      # noqa: E731
    f_one = lambda: one.bp_update(dets[0], nstblz, None, False, reset=False)               # noqa: E731
    f_msd()
    f_one()
    wall = {'msd': [], 'one': []}
    for _ in range(a.reps):                               # alternating: both see the same machine
        for key, fn in (('msd', f_msd), ('one', f_one)):
            c0 = time.perf_counter()
            fn()
            wall[key].append(1e3 * (time.perf_counter() - c0))
    p_msd, k_msd = traced(msd, f_msd)
    p_one, k_one = traced(one, f_one)
    res = {'tool': 'bp_msd_bench', 'M': M, 'K': K, 'na': N, 'nb': N, 'nw': nw, 'ndet': nd, 'nbp': nbp, 'nstblz': nstblz,
           'reps': a.reps,
           'msd': dict(window_ms=float(numpy.median(wall['msd'])), window_ms_min=min(wall['msd']),
                       window_ms_max=max(wall['msd']), **{k + '_ms': v for k, v in p_msd.items()}),
           'single': dict(window_ms=float(numpy.median(wall['one'])), window_ms_min=min(wall['one']),
                          window_ms_max=max(wall['one']), **{k + '_ms': v for k, v in p_one.items()}),
           'four_single_ms': nd * p_one['backward'],
           'loop_backward_ms': p_one['vhs'] + p_one['fields'] + nd * (p_one['products'] + p_one['reortho']),
           'kernels_msd': k_msd, 'kernels_single': k_one}
    res['stacked_over_loop'] = res['msd']['backward_ms'] / res['loop_backward_ms']
    res['stacked_over_four_single'] = res['msd']['backward_ms'] / res['four_single_ms']
    print(json.dumps(res))
    msd.close()
    one.close()


if __name__ == '__main__':
    main()
