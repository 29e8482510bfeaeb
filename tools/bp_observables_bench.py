#!/usr/bin/env python3
"""Milliseconds per back-propagation window of afq_bp_update alone, with the EKT Fock matrices and with the two-body
RDM (afq_bp_update_ext, k_bp_obs.hip), at C3 sizes (M = 100, K = 500, 25+25, 256 walkers) and the EKT at C5
single-determinant sizes (M = 400, K = 2000); model flops of each part and their fraction of the 78.6 TF/s fp64 MFMA
peak.  One JSON line.  The window times are host wall clock around afq_bp_update(_ext): with the two-body RDM they
include allocating the M^4 host array and copying the result out (1.6 GB at M = 100); the kernel's own time is what a
`rocprofv3 --kernel-trace --stats` run of this tool reports for mfma_gemm_kernel<Rdm2Prob>.

  python tools/bp_observables_bench.py [--reps 3] [--c5-walkers 32]
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
from tests.test_gpu_bp_obs import build               # noqa: E402

PEAK = 78.6e12


def ekt_flops(M, K, na, nb, nw):
    """Real flops of the rank-N EKT with symmetric real L: complex x complex multiply-adds at 8 flops, complex x real
    ones (every product with L: the panels and the linear term's two GEMMs) at 4."""
    real = complex_ = 0.0                                                  # multiply-adds
    for N in (na, nb):
        real += nw * K * 2.0 * N * M * M                                  # P = U^T L, R = V L
        complex_ += nw * K * 2.0 * N * N * M                              # W = P V^T, S += W Q
        complex_ += nw * 2.0 * N * M * M                                  # closing V^T S, U S
    complex_ += nw * K * 2.0 * na * (na + nb) * M                         # W' = T U, S' += W' R
    real += K * 2.0 * M ** 3                                               # Y = L Gbar^T, -Y L^T (once per window)
    return 4.0 * real + 8.0 * complex_


def two_rdm_flops(M, nw):
    return 8.0 * M ** 4 * 3 * nw


def setup(M, K, na, nb, nw, nbp=5):
    model, h1e, Lv, rng = build(M, K, na, nb)
    dev = make_device(model, nw)
    ne = na + nb
    dev.set(L.F_PHI, numpy.array([model.psi + 0.1 * (rng.rand(M, ne) + 1j * rng.rand(M, ne)) for _ in range(nw)]))
    dev.set(L.F_OT, dev.calc_overlap())
    dev.bp_configure(nbp)
    for _ in range(nbp):
        dev.propagate(rng.normal(size=(nw, K)), 0.2)
    return model, h1e, dev


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(numpy.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--c5-walkers', type=int, default=32)
    a = ap.parse_args()
    res = {'tool': 'bp_observables_bench'}
    M, K, na, nb, nw = 100, 500, 25, 25, 256
    model, h1e, dev = setup(M, K, na, nb, nw)
    psi = model.psi
    base = timed(lambda: dev.bp_update(psi, 5, None, reset=False), a.reps)
    dev.bp_observables(ekt=True, h1=h1e)
    ekt = timed(lambda: dev.bp_update(psi, 5, None, reset=False, ekt=True), a.reps)
    dev.bp_observables(two_rdm=True)
    two = timed(lambda: dev.bp_update(psi, 5, None, reset=False, two_rdm=True), a.reps)
    dev.close()
    fe, ft = ekt_flops(M, K, na, nb, nw), two_rdm_flops(M, nw)
    res['c3'] = {'M': M, 'K': K, 'na': na, 'nb': nb, 'nw': nw, 'bp_update_ms': base, 'with_ekt_ms': ekt,
                 'with_two_rdm_incl_copy_out_ms': two, 'ekt_ms': ekt - base,
                 'two_rdm_incl_copy_out_ms': two - base,
                 'ekt_model_flop': fe, 'two_rdm_model_flop': ft,
                 'ekt_frac_peak': fe / ((ekt - base) * 1e-3) / PEAK,
                 'two_rdm_incl_copy_out_frac_peak': ft / ((two - base) * 1e-3) / PEAK}
    M, K, na, nb, nw = 400, 2000, 50, 50, a.c5_walkers
    model, h1e, dev = setup(M, K, na, nb, nw, nbp=2)
    psi = model.psi
    base = timed(lambda: dev.bp_update(psi, 5, None, reset=False), a.reps)
    dev.bp_observables(ekt=True, h1=h1e)
    ekt = timed(lambda: dev.bp_update(psi, 5, None, reset=False, ekt=True), a.reps)
    dev.close()
    fe = ekt_flops(M, K, na, nb, nw)
    res['c5'] = {'M': M, 'K': K, 'na': na, 'nb': nb, 'nw': nw, 'bp_update_ms': base, 'with_ekt_ms': ekt,
                 'ekt_ms': ekt - base, 'ekt_model_flop': fe, 'ekt_frac_peak': fe / ((ekt - base) * 1e-3) / PEAK}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
