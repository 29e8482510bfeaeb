#!/usr/bin/env python3
"""Golden fixture for the finite-temperature electron gas at the M = 123 shell (ecut 4.5), from the genuine reference:
the cases of make_golden_thermal_ueg.py (which this imports for its case_a, case_b and margins, and does not change)
where the device needs the far route (walkers: {far_basis: True}).

  thermal_ueg123.npz, the key layout of thermal_ueg.npz:
    a8_*  one ThermalWalker slice by slice: ecut 4.5, M = 123, nup = ndown = 2, rs 1, stack_size 5 (2 bins),
          fb_bound 1.0, beta 0.5, dt 0.05 (10 slices): case a7 of thermal_ueg93.npz one shell further.  a8_G holds the
          slices a8_G_slices (counted from 1) only: the last; every other per-slice quantity (xi, xbar, cmf, cfb, M0,
          weight) is stored for all 10.
    b6_*  ThermalAFQMC over two paths: ecut 4.5, 2 + 2 electrons, beta 0.5, mu 0.245, stack_size 5, 4 walkers,
          pop_control_freq 5.  b6_seed is the first seed from 8 upwards for which the margins of
          make_golden_thermal_ueg.py hold and at least one comb event clones a walker (a parent_ix above 1).

Runs only where the reference is available.

Usage:  python tests/golden/make_golden_thermal_ueg_far.py            (writes the file under tests/golden/)
        python tests/golden/make_golden_thermal_ueg_far.py --check    regenerate into a scratch directory and compare
"""
import os
import shutil
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_thermal_ueg as mt                                     # noqa: E402  (prepares the reference)
from make_golden_thermal_ueg import mg                                   # noqa: E402
from make_golden_thermal_ueg_wide import case_b_first_seed               # noqa: E402

NAME = 'thermal_ueg123.npz'
A123 = (4.5, 2, 1.0, 5, 1.0)              # ecut, nelec per spin, rs, stack_size, fb_bound
B123 = (4.5, 2, 0.5, 0.245, 5, 4)         # ecut, nelec per spin, beta, mu, stack_size, walkers
G_SLICES = numpy.array([10])
MAX_BYTES = 1024 * 1024                   # of a committed file


def make_thermal_ueg123():
    out = {}
    mt.case_a(out, 8, *A123)
    assert out['a8_G'].shape == (10, 2, 123, 123) and out['a8_nclip'] == 0      # nbasis == 123
    out['a8_G_slices'] = G_SLICES
    out['a8_G'] = out['a8_G'][G_SLICES - 1]
    seed = case_b_first_seed(out, 6, B123)
    assert int(out['b6_seed']) == seed and out['b6_blocks'].shape == (3, 12)
    assert numpy.any(out['b6_parent_ix'] > 1)
    mg.save(NAME, out)
    assert os.path.getsize(os.path.join(mg.OUT, NAME)) <= MAX_BYTES
    return seed


if __name__ == '__main__':
    check = '--check' in sys.argv[1:]
    if check:
        import tempfile
        mg.OUT = tempfile.mkdtemp(prefix='golden_check_')
    seed = make_thermal_ueg123()
    status = 0
    if check:
        bad = mg.compare_fixture(NAME, mg.OUT)
        print('%-24s %s' % (NAME, 'identical to the committed fixture' if not bad else 'DIFFERS: ' + '; '.join(bad[:6])))
        status = 1 if bad else 0
        shutil.rmtree(mg.OUT, ignore_errors=True)
    else:
        print('%-24s %d bytes, seed %d' % (NAME, os.path.getsize(os.path.join(mg.OUT, NAME)), seed))
    sys.exit(status)
