#!/usr/bin/env python3
"""Golden fixture for the finite-temperature electron gas at the M = 57 shell (ecut 2.5), from the genuine reference:
the cases of make_golden_thermal_ueg.py (which this imports for its case_a, case_b and margins, and does not change) one
shell further, where the device needs the streamed Green's function (walkers: {streamed_greens: True}).

  thermal_ueg57.npz, the key layout of thermal_ueg.npz:
    a5_*  one ThermalWalker slice by slice: ecut 2.5, M = 57, nup = ndown = 2, rs 1, stack_size 5 (2 bins),
          fb_bound 1.0, beta 0.5, dt 0.05 (10 slices).  G per slice would make the file larger than a committed file
          may be, so a5_G holds the ODD slices only (the 1st, 3rd, .. 9th: a5_G_slices, counted from 1); every other
          per-slice quantity (xi, xbar, cmf, cfb, M0, weight) is stored for all 10.
    b4_*  ThermalAFQMC over two paths: ecut 2.5, 2 + 2 electrons, beta 0.5, mu 0.245, stack_size 5, 6 walkers,
          pop_control_freq 5.  b4_seed is the first seed from 8 upwards for which the margins of
          make_golden_thermal_ueg.py hold (no comb tooth within 1e-6 of a cumulative weight, no cosine within 1e-6 of 0)
          and at least one comb event clones a walker (a parent_ix above 1).

Runs only where the reference is available.

Usage:  python tests/golden/make_golden_thermal_ueg57.py            (writes tests/golden/thermal_ueg57.npz)
        python tests/golden/make_golden_thermal_ueg57.py --check    regenerate into a scratch directory and compare
"""
import os
import shutil
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_thermal_ueg as mt                                     # noqa: E402  (prepares the reference)
from make_golden_thermal_ueg import mg                                   # noqa: E402

NAME = 'thermal_ueg57.npz'
A_CASE = (2.5, 2, 1.0, 5, 1.0)            # ecut, nelec per spin, rs, stack_size, fb_bound
B_CASE = (2.5, 2, 0.5, 0.245, 5, 6)       # ecut, nelec per spin, beta, mu, stack_size, walkers
FIRST_SEED, LAST_SEED = 8, 64
MAX_BYTES = 1024 * 1024                   # of a committed file


def case_b_first_seed(out):
    """case_b at the first seed whose run keeps the margins (they are case_b's own assertions) and clones a walker."""
    for seed in range(FIRST_SEED, LAST_SEED + 1):
        trial = {}
        try:
            mt.case_b(trial, 4, *(B_CASE + (seed,)))
        except AssertionError as e:
            print('seed %d: %s' % (seed, e))
            del mt.COS[:]
            continue
        if not numpy.any(trial['b4_parent_ix'] > 1):
            print('seed %d: no comb event clones a walker' % seed)
            continue
        out.update(trial)
        return seed
    raise SystemExit('no seed in %d .. %d keeps the margins and clones a walker' % (FIRST_SEED, LAST_SEED))


def make_thermal_ueg57():
    out = {}
    mt.case_a(out, 5, *A_CASE)
    assert out['a5_G'].shape == (10, 2, 57, 57) and out['a5_nclip'] == 0
    out['a5_G_slices'] = numpy.arange(1, 11, 2)
    out['a5_G'] = out['a5_G'][out['a5_G_slices'] - 1]
    seed = case_b_first_seed(out)
    assert int(out['b4_seed']) == seed and out['b4_blocks'].shape == (3, 12)
    mg.save(NAME, out)
    assert os.path.getsize(os.path.join(mg.OUT, NAME)) <= MAX_BYTES
    return seed


if __name__ == '__main__':
    check = '--check' in sys.argv[1:]
    if check:
        import tempfile
        mg.OUT = tempfile.mkdtemp(prefix='golden_check_')
    seed = make_thermal_ueg57()
    if check:
        bad = mg.compare_fixture(NAME, mg.OUT)
        print('%-24s %s' % (NAME, 'identical to the committed fixture' if not bad else 'DIFFERS: ' + '; '.join(bad[:6])))
        shutil.rmtree(mg.OUT, ignore_errors=True)
        sys.exit(1 if bad else 0)
    print('%-24s %d bytes, seed %d' % (NAME, os.path.getsize(os.path.join(mg.OUT, NAME)), seed))
