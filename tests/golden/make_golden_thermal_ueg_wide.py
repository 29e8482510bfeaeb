#!/usr/bin/env python3
"""Golden fixtures for the finite-temperature electron gas at the M = 81 and M = 93 shells (ecut 3.0 and 4.0), from the
genuine reference: the cases of make_golden_thermal_ueg.py (which this imports for its case_a, case_b and margins, and
does not change) where the device needs the wide route (walkers: {wide_basis: True}).

  thermal_ueg81.npz, the key layout of thermal_ueg.npz:
    a6_*  one ThermalWalker slice by slice: ecut 3.0, M = 81, nup = ndown = 2, rs 1, stack_size 5 (2 bins),
          fb_bound 1.0, beta 0.5, dt 0.05 (10 slices).  a6_G holds the slices a6_G_slices (counted from 1) only: one in
          the middle of the first bin and the last; every other per-slice quantity (xi, xbar, cmf, cfb, M0, weight) is
          stored for all 10.
    b5_*  ThermalAFQMC over two paths: ecut 3.0, 2 + 2 electrons, beta 0.5, mu 0.245, stack_size 5, 6 walkers,
          pop_control_freq 5.  b5_seed is the first seed from 8 upwards for which the margins of
          make_golden_thermal_ueg.py hold and at least one comb event clones a walker (a parent_ix above 1).
  thermal_ueg93.npz:
    a7_*  as a6 at ecut 4.0, M = 93.

Runs only where the reference is available.

Usage:  python tests/golden/make_golden_thermal_ueg_wide.py            (writes both files under tests/golden/)
        python tests/golden/make_golden_thermal_ueg_wide.py --check    regenerate into a scratch directory and compare
"""
import os
import shutil
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_thermal_ueg as mt                                     # noqa: E402  (prepares the reference)
from make_golden_thermal_ueg import mg                                   # noqa: E402

NAME81, NAME93 = 'thermal_ueg81.npz', 'thermal_ueg93.npz'
A81 = (3.0, 2, 1.0, 5, 1.0)               # ecut, nelec per spin, rs, stack_size, fb_bound
A93 = (4.0, 2, 1.0, 5, 1.0)
B81 = (3.0, 2, 0.5, 0.245, 5, 6)          # ecut, nelec per spin, beta, mu, stack_size, walkers
G_SLICES = numpy.array([3, 10])
FIRST_SEED, LAST_SEED = 8, 64
MAX_BYTES = 1024 * 1024                   # of a committed file


def case_a_two_slices(out, k, case, M):
    mt.case_a(out, k, *case)
    pre = 'a%d_' % k
    assert out[pre + 'G'].shape == (10, 2, M, M) and out[pre + 'nclip'] == 0
    out[pre + 'G_slices'] = G_SLICES
    out[pre + 'G'] = out[pre + 'G'][G_SLICES - 1]


def case_b_first_seed(out, k, case):
    """case_b at the first seed whose run keeps the margins (they are case_b's own assertions) and clones a walker."""
    for seed in range(FIRST_SEED, LAST_SEED + 1):
        trial = {}
        try:
            mt.case_b(trial, k, *(case + (seed,)))
        except AssertionError as e:
            print('seed %d: %s' % (seed, e))
            del mt.COS[:]
            continue
        if not numpy.any(trial['b%d_parent_ix' % k] > 1):
            print('seed %d: no comb event clones a walker' % seed)
            continue
        out.update(trial)
        return seed
    raise SystemExit('no seed in %d .. %d keeps the margins and clones a walker' % (FIRST_SEED, LAST_SEED))


def make_thermal_ueg81():
    out = {}
    case_a_two_slices(out, 6, A81, 81)
    seed = case_b_first_seed(out, 5, B81)
    assert int(out['b5_seed']) == seed and out['b5_blocks'].shape == (3, 12)
    mg.save(NAME81, out)
    assert os.path.getsize(os.path.join(mg.OUT, NAME81)) <= MAX_BYTES
    return seed


def make_thermal_ueg93():
    out = {}
    case_a_two_slices(out, 7, A93, 93)
    mg.save(NAME93, out)
    assert os.path.getsize(os.path.join(mg.OUT, NAME93)) <= MAX_BYTES


if __name__ == '__main__':
    check = '--check' in sys.argv[1:]
    if check:
        import tempfile
        mg.OUT = tempfile.mkdtemp(prefix='golden_check_')
    seed = make_thermal_ueg81()
    make_thermal_ueg93()
    status = 0
    for name in (NAME81, NAME93):
        if check:
            bad = mg.compare_fixture(name, mg.OUT)
            print('%-24s %s' % (name, 'identical to the committed fixture' if not bad else 'DIFFERS: ' + '; '.join(bad[:6])))
            status |= 1 if bad else 0
        else:
            print('%-24s %d bytes%s' % (name, os.path.getsize(os.path.join(mg.OUT, name)),
                                        ', seed %d' % seed if name == NAME81 else ''))
    if check:
        shutil.rmtree(mg.OUT, ignore_errors=True)
    sys.exit(status)
