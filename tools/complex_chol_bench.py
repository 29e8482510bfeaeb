#!/usr/bin/env python3
"""C3-size step timing with Hermitian COMPLEX Cholesky vectors (M=100, K=500, 25+25, RHF trial, 256 walkers), next to
the same system with real vectors in the same run.  Prints one JSON line.

One flop model for every row: the matrix-pipe flops the library reports for the last launch of a kernel kind
(afq_kernel_issued_flops: executed MFMA work, padding included), over the traced launch time, as a fraction of the
78.6 TF/s fp64 peak.

  python tools/complex_chol_bench.py [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pauxy_amd import _lib as L                                    # noqa: E402
from pauxy_amd import systems, trial as trial_mod                  # noqa: E402
from pauxy_amd.device import AfqDevice                             # noqa: E402
from pauxy_amd.propagation import setup                            # noqa: E402

M, K, N, NW, DT = 100, 500, 25, 256, 0.005
PEAK = 78.6e12
KINDS = {'propagator': L.K_PROPAGATOR, 'exchange': L.K_EXCHANGE, 'vhs': L.K_VHS, 'force_bias': L.K_FORCE_BIAS}


def system(cplx):
    s = systems.synthetic_generic(M, K, (N, N), seed=7)
    if not cplx:
        return s
    rng = numpy.random.RandomState(7)
    L3 = s.hs_pot.T.reshape(K, M, M)
    A = rng.normal(size=(K, M, M)) * (0.05 * numpy.abs(L3).mean())
    Lc = L3 + 1j * 0.5 * (A - A.transpose(0, 2, 1))          # Hermitian: real symmetric + i antisymmetric
    return systems.Generic((N, N), s.H1, numpy.ascontiguousarray(Lc.reshape(K, M * M).T), s.ecore)


def run(cplx, steps, warmup):
    s = system(cplx)
    t = trial_mod.rhf_trial_generic(s)
    BH1, mf = setup.generic_propagator_arrays(s, t, DT)
    dev = AfqDevice(0)
    dev.set_system_generic(s.hs_pot, numpy.asarray(t._rchol)[:2 * N * M], numpy.asarray(s.H1, dtype=complex),
                           s.ecore, N, N)
    dev.set_trial(t.psi)
    dev.set_propagator(BH1, mf, DT)
    dev.walkers_alloc(NW)
    dev.set(L.F_PHI, numpy.array([t.psi] * NW))
    dev.set(L.F_OT, dev.calc_overlap())
    rng = numpy.random.RandomState(1)
    xi = rng.normal(size=(NW, K))

    def step(i):
        # bench.py's cadence without population control: re-orthogonalisation and energy every 10 steps
        dev.propagate(xi, -1.0)
        if i % 10 == 9:
            dev.reortho(fetch=False)
            dev.greens()
            dev.local_energy(fetch=False)

    for i in range(warmup):
        step(i)
    dev.sync()
    dev.counters(reset=True, n=8)
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    dev.sync()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    cnt = [int(x) for x in dev.counters(n=8)]
    dev.kernel_trace(True)
    for i in range(10):
        step(i)
    dev.sync()
    rows = {}
    for name, k in KINDS.items():
        ts = dev.kernel_trace_get(k)
        if len(ts) == 0:
            continue
        us = float(numpy.median(ts)) * 1e3
        fl = dev.kernel_issued_flops(k)
        rows[name] = {'us': round(us, 2), 'issued_gflop': round(fl / 1e9, 3),
                      'frac_peak': round(fl / (us * 1e-6) / PEAK, 4) if fl > 0 else None}
    dev.kernel_trace(False)
    dev.close()
    return {'ms_per_step': round(ms, 4), 'walker_steps_per_s': round(NW * 1e3 / ms, 1), 'kernels': rows,
            'counters': {'closed_deal_walker_steps': cnt[3], 'one_spin_exchange': cnt[4],
                         'one_spin_greens': cnt[5], 'closed_gemm_chain_steps': cnt[7]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    c = run(True, a.steps, a.warmup)
    r = run(False, a.steps, a.warmup)
    vr = c['kernels'].get('vhs', {}).get('us'), r['kernels'].get('vhs', {}).get('us')
    print(json.dumps({'config': 'C3 Hermitian complex L', 'M': M, 'K': K, 'nelec': [N, N], 'nw': NW,
                      'flop_model': 'afq_kernel_issued_flops (executed MFMA work) / traced launch time / 78.6 TF/s',
                      'complex': c, 'real_same_run': r,
                      'vhs_ratio_complex_to_real': round(vr[0] / vr[1], 3) if all(vr) else None}))


if __name__ == '__main__':
    main()
