#!/usr/bin/env python3
"""Cost of the back-propagated pairing correlations (two_rdm: 'pairing', k_pair.hip) at the C4 sizes: Hubbard 16 x 16 at
half filling, discrete fields, 256 walkers (256 Green's functions of M = 256), the five lattice bonds.  Prints one JSON
line.

  pair_wsum_us   k_pair_wsum: pair_tile_kernel<true> + corr_combine_kernel (k_sum_chunks), device event pairs around every launch
                 (afq_launch_trace), summed per window; median, min and max over `--windows` windows
  corr_wsum_us   k_corr_wsum (corr_diag_kernel + corr_tile_kernel<true> + corr_combine_kernel) on the same G_bp, the
                 windows of the two modes alternating on one handle (reset=False: the same history every time)
  bytes_min      what the sum has to move: reads 2 M^2 16 n, writes nb^2 M^2 16
  bytes_moved    what the kernels request, from the shapes: per Green's function and tile the G_0 elements once per
                 block of bond pairs and nb^2 gathered G_1 elements; the partial sums of every chunk written, read again
                 and the result written
Warm-up windows of both modes come first.  The event pairs cost a few microseconds of bubble per launch and are around
single kernels: they time the kernels, not the window.

  python tools/pairing_bench.py [--windows 10] [--warmup 3] [--nbp 4]
"""
import argparse
import json
import os
import sys

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from corr_bench import make                                        # noqa: E402
from pauxy_amd import _lib as L                                    # noqa: E402
from pauxy_amd.estimators.pairing import lattice_bonds             # noqa: E402

PT, PB, PAIR_WCH = 16, 5, 64                                       # k_pair.hip: tile edge, bonds per block, chunk
PAIR = ('pair_tile_kernel', 'corr_combine_kernel')                 # (the launch trace's names, up to template arguments;
CORR = ('corr_diag_kernel', 'corr_tile_kernel', 'corr_combine_kernel')     # both sums add their chunks with one kernel)


def traced(dev, psi, mode, names):
    """One window in `mode` under the launch trace -> microseconds per kernel of `names` (0 where it did not run)."""
    dev.bp_observables(two_rdm=mode)
    dev.sync()
    dev.launch_trace(True)
    dev.bp_update(psi, 5, None, False, reset=False, two_rdm=True)
    got = dev.launch_trace_get()
    dev.launch_trace(False)
    return [1e3 * sum(ms for name, (cnt, ms) in got.items() if name.startswith(k)) for k in names]


def stats(rows, names):
    tot = [sum(r) for r in rows]
    out = {'median': float(numpy.median(tot)), 'min': float(min(tot)), 'max': float(max(tot))}
    for i, k in enumerate(names):
        out[k] = float(numpy.median([r[i] for r in rows]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=16)
    ap.add_argument('--walkers', type=int, default=256)
    ap.add_argument('--nbp', type=int, default=4)
    ap.add_argument('--windows', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    dev, psi, rng = make(a.nx, a.nx, a.walkers)
    dev.bp_configure(a.nbp)
    for step in range(a.nbp):
        dev.hirsch_kinetic()
        dev.hirsch_two_body(rng.random_sample((dev.nw, dev.M)))
        dev.hirsch_finish(0.0)
    nbr = lattice_bonds(a.nx, a.nx)[0]
    dev.set_pairing_bonds(nbr)
    M, nb = dev.M, len(nbr)
    pair, corr = [], []
    for k in range(a.warmup + a.windows):
        p, c = traced(dev, psi, 'pairing', PAIR), traced(dev, psi, 'correlation', CORR)
        if k >= a.warmup:
            pair.append(p)
            corr.append(c)
    n = int(numpy.count_nonzero(dev.get(L.F_WEIGHT)))
    nchunk, nblk = -(-a.walkers // PAIR_WCH), -(-nb // PB)
    out_len = 16 * nb * nb * M * M
    res = {'system': 'Hubbard %dx%d' % (a.nx, a.nx), 'M': M, 'nb': nb, 'greens_functions': n, 'nbp': a.nbp,
           'windows': a.windows, 'pair_wsum_us': stats(pair, PAIR), 'corr_wsum_us': stats(corr, CORR),
           'bytes_min': 2 * M * M * 16 * n + out_len,
           'bytes_moved': 16 * M * M * n * (nblk * nblk + nb * nb) + (out_len * (2 * nchunk + 1) if nchunk > 1 else out_len)}
    res['pair_over_corr'] = res['pair_wsum_us']['median'] / res['corr_wsum_us']['median']
    res['bytes_moved_over_min'] = res['bytes_moved'] / res['bytes_min']
    res['min_bytes_per_s'] = res['bytes_min'] / (1e-6 * res['pair_wsum_us']['median'])
    res['moved_bytes_per_s'] = res['bytes_moved'] / (1e-6 * res['pair_wsum_us']['median'])
    dev.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
