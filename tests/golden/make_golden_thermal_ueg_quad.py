#!/usr/bin/env python3
"""Golden fixture for the finite-temperature electron gas at the M = 147 shell (ecut 5.0), from the genuine reference:
the cases of make_golden_thermal_ueg.py (which this imports for its case_a, case_b and margins, and does not change)
where the device needs the quad route (walkers: {quad_basis: True}).

  thermal_ueg147.npz, the key layout of thermal_ueg.npz:
    a9_*  one ThermalWalker slice by slice: ecut 5.0, M = 147, nup = ndown = 2, rs 1, stack_size 5 (2 bins),
          fb_bound 1.0, beta 0.5, dt 0.05 (10 slices): case a8 of thermal_ueg123.npz one shell further.  a9_G holds the
          slices a9_G_slices (counted from 1) only: the last; every other per-slice quantity (xi, xbar, cmf, cfb, M0,
          weight) is stored for all 10.
    b7_*  ThermalAFQMC over two paths: ecut 5.0, 2 + 2 electrons, beta 0.5, mu 0.245, stack_size 5, 4 walkers,
          pop_control_freq 5.  b7_seed is the first seed from 8 upwards for which the margins of
          make_golden_thermal_ueg.py hold and at least one comb event clones a walker (a parent_ix above 1): both are
          checked here, on the CPU (case_b_first_seed).  With 4 walkers at beta 0.5 the weights stay close and a clone
          is rare: every one of the seeds 8 .. SEARCHED = 95 keeps the margins and runs to the end, and in every one of
          them the parents of every comb event are 1, 1, 1, 1 (recorded when the fixture was made: no seed of them
          fails for another reason); six seconds each, so a plain run starts behind them and --search runs them
          again.  The search rebinds FIRST_SEED / LAST_SEED of make_golden_thermal_ueg_wide for its call and puts
          them back.

Runs only where the reference is available.

Usage:  python tests/golden/make_golden_thermal_ueg_quad.py            (writes the file under tests/golden/)
        python tests/golden/make_golden_thermal_ueg_quad.py --check    regenerate into a scratch directory and compare
        python tests/golden/make_golden_thermal_ueg_quad.py --search   either, with the seed search from 8
"""
import os
import shutil
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_thermal_ueg as mt                                     # noqa: E402  (prepares the reference)
import make_golden_thermal_ueg_wide as mw                                # noqa: E402
from make_golden_thermal_ueg import mg                                   # noqa: E402
from make_golden_thermal_ueg_wide import case_b_first_seed               # noqa: E402
from make_golden_thermal_ueg_far import A123, B123, MAX_BYTES            # noqa: E402  (the cases one shell below)

NAME = 'thermal_ueg147.npz'
A147 = (5.0,) + A123[1:]                  # ecut, nelec per spin, rs, stack_size, fb_bound
B147 = (5.0,) + B123[1:]                  # ecut, nelec per spin, beta, mu, stack_size, walkers
G_SLICES = numpy.array([10])
SEARCHED, LAST_SEED = 95, 160            # of the seeds from mw.FIRST_SEED to SEARCHED none clones a walker


def make_thermal_ueg147(search=False):
    out = {}
    mt.case_a(out, 9, *A147)
    assert out['a9_G'].shape == (10, 2, 147, 147) and out['a9_nclip'] == 0      # nbasis == 147
    out['a9_G_slices'] = G_SLICES
    out['a9_G'] = out['a9_G'][G_SLICES - 1]
    first, last = mw.FIRST_SEED, mw.LAST_SEED
    mw.FIRST_SEED, mw.LAST_SEED = (first if search else SEARCHED + 1), LAST_SEED
    try:
        seed = case_b_first_seed(out, 7, B147)
    finally:
        mw.FIRST_SEED, mw.LAST_SEED = first, last
    assert seed > SEARCHED
    assert int(out['b7_seed']) == seed and out['b7_blocks'].shape == (3, 12)
    assert numpy.any(out['b7_parent_ix'] > 1)
    mg.save(NAME, out)
    assert os.path.getsize(os.path.join(mg.OUT, NAME)) <= MAX_BYTES, os.path.getsize(os.path.join(mg.OUT, NAME))
    return seed


if __name__ == '__main__':
    check = '--check' in sys.argv[1:]
    if check:
        import tempfile
        mg.OUT = tempfile.mkdtemp(prefix='golden_check_')
    seed = make_thermal_ueg147(search='--search' in sys.argv[1:])
    status = 0
    if check:
        bad = mg.compare_fixture(NAME, mg.OUT)
        print('%-24s %s' % (NAME, 'identical to the committed fixture' if not bad else 'DIFFERS: ' + '; '.join(bad[:6])))
        status = 1 if bad else 0
        shutil.rmtree(mg.OUT, ignore_errors=True)
    else:
        print('%-24s %d bytes, seed %d' % (NAME, os.path.getsize(os.path.join(mg.OUT, NAME)), seed))
    sys.exit(status)
