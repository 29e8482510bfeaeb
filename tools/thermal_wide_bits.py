#!/usr/bin/env python3
"""G and det of the complex wide route (AFQ_THERMAL_WIDE, thermal_cgreens_wide_kernel) on fixed uploaded stacks, saved
so that two builds of the library can be compared bit for bit: Hubbard chains of M = 19 and M = 81 with continuous
fields, 2 walkers, 3 bins, slices 0 and 3.

  python tools/thermal_wide_bits.py --out A.npz           on one build (a checkout of another commit runs its own copy
                                                          of this file, or this one: it needs only tests/ and pauxy_amd)
  python tools/thermal_wide_bits.py --compare A.npz B.npz  prints per array whether the 64-bit patterns are equal; exit
                                                          status 1 if any differs
"""
import argparse
import os
import sys

import numpy

sys.path.insert(0, os.getcwd())


def record(out):
    from pauxy_amd import _lib as L
    from tests.test_gpu_thermal_wide import BIT, chain, complex_stack
    res = {}
    for M in (19, 81):
        stack = complex_stack(M, 2, 3, 2, 5)
        dev = chain(M, 6).device(2, 2, BIT)
        try:
            dev.set(L.F_THERMAL_STACK, stack)
            for s in (0, 3):
                dev.thermal_greens(s)
                res['G_%d_%d' % (M, s)] = dev.get(L.F_THERMAL_G)
                res['det_%d_%d' % (M, s)] = dev.get(L.F_THERMAL_DET)
        finally:
            dev.close()
    numpy.savez(out, **res)
    print('saved', out, sorted(res))


def compare(a, b):
    a, b = numpy.load(a), numpy.load(b)
    assert sorted(a.files) == sorted(b.files)
    bad = 0
    for k in sorted(a.files):
        same = numpy.array_equal(a[k].view(numpy.uint64), b[k].view(numpy.uint64))
        print(k, 'bit-equal' if same else 'DIFFERS, largest difference %.3e' % numpy.max(numpy.abs(a[k] - b[k])))
        bad += not same
    print('all bit-equal' if not bad else '%d arrays differ' % bad)
    return 1 if bad else 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--compare', nargs=2, default=None)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    record(a.out or 'thermal_wide_bits.npz')
