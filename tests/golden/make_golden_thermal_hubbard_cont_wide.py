#!/usr/bin/env python3
"""Golden fixture for the Hubbard model with continuous fields beyond 63 sites, from the genuine reference: the cases of
make_golden_thermal_hubbard_cont.py (which this imports for its case_a, case_b and margins, and does not change) where
the device needs the wide route (walkers: {wide_basis: True}).

  thermal_hubbard_cont_wide.npz, the key layout of thermal_hubbard_cont.npz:
    a8_*  one ThermalWalker slice by slice on 8 x 8 (M = 64: the last M with an empty second column per lane), 28 + 28
          electrons, U 4, mu 1, dt 0.05, stack_size 5 (2 bins), 10 slices: xi, xbar, cmf, cfb, M0 and the weight for
          every slice, G behind the last (a8_G_last).
    a9_*  the same on a chain of 65 sites (nx 65, ny 1: the first M with a second column).
    b2_*  ThermalAFQMC over two paths on 8 x 8 with 4 walkers, beta 1, stack_size 5, pop_control_freq 5, seed 7.

Runs only where the reference is available.

Usage:  python tests/golden/make_golden_thermal_hubbard_cont_wide.py            (writes the file under tests/golden/)
        python tests/golden/make_golden_thermal_hubbard_cont_wide.py --check    regenerate into a scratch directory and compare
"""
import os
import shutil
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_thermal_hubbard_cont as mh                            # noqa: E402  (prepares the reference)
from make_golden_thermal_hubbard_cont import mg                          # noqa: E402

NAME = 'thermal_hubbard_cont_wide.npz'
A_CASES = {8: (8, 8, 28, 4.0, 1.0, 0.05, 5, 15), 9: (65, 1, 28, 4.0, 1.0, 0.05, 5, 16)}   # as mh.A_CASES
B_CASES = {2: (8, 8, 28, 5, 4, 7)}                                                          # as mh.B_CASES
MAX_BYTES = 1024 * 1024                   # of a committed file


def make_thermal_hubbard_cont_wide():
    out = {}
    for k, case in A_CASES.items():
        mh.case_a(out, k, *case)
        assert 'a%d_G' % k not in out and out['a%d_G_last' % k].shape == (2, case[0] * case[1], case[0] * case[1])
    for k, case in B_CASES.items():
        mh.case_b(out, k, *case)
    mg.save(NAME, out)
    assert os.path.getsize(os.path.join(mg.OUT, NAME)) <= MAX_BYTES


if __name__ == '__main__':
    check = '--check' in sys.argv[1:]
    if check:
        import tempfile
        mg.OUT = tempfile.mkdtemp(prefix='golden_check_')
    make_thermal_hubbard_cont_wide()
    if check:
        bad = mg.compare_fixture(NAME, mg.OUT)
        print('%-32s %s' % (NAME, 'identical to the committed fixture' if not bad else 'DIFFERS: ' + '; '.join(bad[:6])))
        shutil.rmtree(mg.OUT, ignore_errors=True)
        sys.exit(1 if bad else 0)
    print('%-32s %d bytes' % (NAME, os.path.getsize(os.path.join(mg.OUT, NAME))))
