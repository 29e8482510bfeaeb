#!/usr/bin/env python3
"""Golden fixture for the Hubbard model with continuous fields beyond 95 sites, from the genuine reference: the cases of
make_golden_thermal_hubbard_cont.py (which this imports for its case_a, case_b and margins, and does not change) where
the device needs the far route (walkers: {far_basis: True}).

  thermal_hubbard_cont_far.npz, the key layout of thermal_hubbard_cont.npz but for what is said here:
    a10_*  one ThermalWalker slice by slice on 8 x 16 (M = 128: the bound itself, pitch 129), 56 + 56 electrons, U 4,
           mu 1, dt 0.05, stack_size 5 (2 bins), 10 slices: xi, xbar, cmf, cfb, M0 and the weight for every slice, G
           behind the last (a10_G_last).  To stay below the size of a committed file a10_dmat, a10_dmat_inv and a10_BH1
           hold the one spin [1, M, M] (both spins are asserted equal here) and the trial's G is not stored (a10_M00 is).
    b3_*   ThermalAFQMC over two paths on 10 x 10 with 4 walkers, 44 + 44 electrons, beta 1, stack_size 5,
           pop_control_freq 5, seed 7.

Runs only where the reference is available.

Usage:  python tests/golden/make_golden_thermal_hubbard_cont_far.py            (writes the file under tests/golden/)
        python tests/golden/make_golden_thermal_hubbard_cont_far.py --check    regenerate into a scratch directory and compare
"""
import os
import shutil
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_thermal_hubbard_cont as mh                            # noqa: E402  (prepares the reference)
from make_golden_thermal_hubbard_cont import mg                          # noqa: E402

NAME = 'thermal_hubbard_cont_far.npz'
A_CASES = {10: (8, 16, 56, 4.0, 1.0, 0.05, 5, 17)}                       # as mh.A_CASES
B_CASES = {3: (10, 10, 44, 5, 4, 7)}                                      # as mh.B_CASES
MAX_BYTES = 1024 * 1024                   # of a committed file


def make_thermal_hubbard_cont_far():
    out = {}
    for k, case in A_CASES.items():
        mh.case_a(out, k, *case)
        pre, M = 'a%d_' % k, case[0] * case[1]
        assert pre + 'G' not in out and out[pre + 'G_last'].shape == (2, M, M)
        for q in ('dmat', 'dmat_inv', 'BH1'):
            assert out[pre + q].shape == (2, M, M) and numpy.array_equal(out[pre + q][0], out[pre + q][1])
            out[pre + q] = out[pre + q][:1]
        del out[pre + 'G0']
    for k, case in B_CASES.items():
        mh.case_b(out, k, *case)
    mg.save(NAME, out)
    assert os.path.getsize(os.path.join(mg.OUT, NAME)) <= MAX_BYTES


if __name__ == '__main__':
    check = '--check' in sys.argv[1:]
    if check:
        import tempfile
        mg.OUT = tempfile.mkdtemp(prefix='golden_check_')
    make_thermal_hubbard_cont_far()
    if check:
        bad = mg.compare_fixture(NAME, mg.OUT)
        print('%-32s %s' % (NAME, 'identical to the committed fixture' if not bad else 'DIFFERS: ' + '; '.join(bad[:6])))
        shutil.rmtree(mg.OUT, ignore_errors=True)
        sys.exit(1 if bad else 0)
    print('%-32s %d bytes' % (NAME, os.path.getsize(os.path.join(mg.OUT, NAME))))
