#!/usr/bin/env python3
"""Golden fixture for the Hubbard model with continuous fields beyond 128 sites, from the genuine reference: the cases of
make_golden_thermal_hubbard_cont.py (which this imports for its case_a, case_b and margins, and does not change) where
the device needs the quad route (walkers: {quad_basis: True}).

  thermal_hubbard_cont_quad.npz, the key layout of thermal_hubbard_cont_far.npz but for what is said here:
    a11_*  one ThermalWalker slice by slice on 16 x 16 (M = 256: the bound itself, pitch 257), 112 + 112 electrons, U 4,
           mu 1, dt 0.05, stack_size 5 (2 bins), 10 slices: xi, xbar, cmf, cfb, M0 and the weight for every slice.  A
           [2, 256, 256] complex matrix is 2 MiB, so of what the walker holds behind the last slice the file keeps the
           rows a11_rows = 0, 63, 64, 127, 128, 191, 192, 255 (a row crosses all four column classes of the lanes;
           the rows are the ends of the four classes): a11_G_last [2, 8, M], a11_bins_last [2 bins, 2, 8, M] and
           a11_right_last [2, 8, M].  a11_dmat, a11_dmat_inv and a11_BH1 hold the one spin [1, M, M] (both spins are
           asserted equal here) and the trial's G is not stored (a11_M00 is).
    b4_*   ThermalAFQMC over two paths on 12 x 12 (M = 144) with 4 walkers, 64 + 64 electrons, beta 1, stack_size 5,
           pop_control_freq 5; b4_seed is the first seed from 7 upwards for which case_b's margins hold.  No matrix of
           the driver run is stored.

Runs only where the reference is available.

Usage:  python tests/golden/make_golden_thermal_hubbard_cont_quad.py            (writes the file under tests/golden/)
        python tests/golden/make_golden_thermal_hubbard_cont_quad.py --check    regenerate into a scratch directory and compare
"""
import os
import shutil
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_thermal_hubbard_cont as mh                            # noqa: E402  (prepares the reference)
from make_golden_thermal_hubbard_cont import mg                          # noqa: E402
from make_golden_thermal_hubbard_cont_far import A_CASES as FAR_A, B_CASES as FAR_B, MAX_BYTES    # noqa: E402

NAME = 'thermal_hubbard_cont_quad.npz'
A_CASES = {11: (16, 16, 112) + FAR_A[10][3:]}                            # as mh.A_CASES: 8 x 16 of the far file, doubled
B_CASES = {4: (12, 12, 64) + FAR_B[3][3:5]}                              # as mh.B_CASES less the seed
ROWS = numpy.array([0, 63, 64, 127, 128, 191, 192, 255])
FIRST_SEED, LAST_SEED = 7, 64


def case_a_rows(out, k, case):
    """mh.case_a, and of the walker it made the rows ROWS of G, the bins and right behind the last slice."""
    made = []
    walker_class = mh.ThermalWalker

    def keep(*a, **kw):
        made.append(walker_class(*a, **kw))
        return made[-1]
    mh.ThermalWalker = keep
    try:
        mh.case_a(out, k, *case)
    finally:
        mh.ThermalWalker = walker_class
    walker, = made
    pre, M = 'a%d_' % k, case[0] * case[1]
    assert pre + 'G' not in out and out[pre + 'G_last'].shape == (2, M, M) and numpy.array_equal(out[pre + 'G_last'], walker.G)
    for q in ('dmat', 'dmat_inv', 'BH1'):
        assert out[pre + q].shape == (2, M, M) and numpy.array_equal(out[pre + q][0], out[pre + q][1])
        out[pre + q] = out[pre + q][:1]
    del out[pre + 'G0']
    stack = numpy.asarray(walker.stack.stack)
    right = numpy.asarray(walker.stack.right)[-1]                  # (the reference keeps one per bin: the last bin's is current)
    assert stack.shape == (mh.NSLICE // case[6], 2, M, M) and right.shape == (2, M, M)
    out[pre + 'rows'] = ROWS
    out[pre + 'G_last'] = out[pre + 'G_last'][:, ROWS]
    out[pre + 'bins_last'] = stack[:, :, ROWS].astype(numpy.complex128)
    out[pre + 'right_last'] = right[:, ROWS].astype(numpy.complex128)


def case_b_first_seed(out, k, case):
    for seed in range(FIRST_SEED, LAST_SEED + 1):
        trial = {}
        try:
            mh.case_b(trial, k, *(case + (seed,)))
        except AssertionError as e:
            print('seed %d: %s' % (seed, e))
            del mh.COS[:]
            continue
        out.update(trial)
        return seed
    raise SystemExit('no seed in %d .. %d keeps the margins' % (FIRST_SEED, LAST_SEED))


def make_thermal_hubbard_cont_quad():
    out = {}
    for k, case in A_CASES.items():
        case_a_rows(out, k, case)
    for k, case in B_CASES.items():
        seed = case_b_first_seed(out, k, case)
        assert int(out['b%d_seed' % k]) == seed
    mg.save(NAME, out)
    assert os.path.getsize(os.path.join(mg.OUT, NAME)) <= MAX_BYTES, os.path.getsize(os.path.join(mg.OUT, NAME))


if __name__ == '__main__':
    check = '--check' in sys.argv[1:]
    if check:
        import tempfile
        mg.OUT = tempfile.mkdtemp(prefix='golden_check_')
    make_thermal_hubbard_cont_quad()
    if check:
        bad = mg.compare_fixture(NAME, mg.OUT)
        print('%-32s %s' % (NAME, 'identical to the committed fixture' if not bad else 'DIFFERS: ' + '; '.join(bad[:6])))
        shutil.rmtree(mg.OUT, ignore_errors=True)
        sys.exit(1 if bad else 0)
    print('%-32s %d bytes' % (NAME, os.path.getsize(os.path.join(mg.OUT, NAME))))
