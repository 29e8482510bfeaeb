#!/usr/bin/env python3
"""The cases of the far fixtures (thermal_ueg123.npz, thermal_hubbard_cont_far.npz) through the extended-precision
restatements of the tests, stored so that the GPU tests can hold them to the accuracy rule without running
numpy.clongdouble themselves, as make_thermal_wide_ext.py does for the wide fixtures.  One file per fixture, each below
the size of a committed file:

  thermal_ueg123_ext.npz  a8_<q>_hi / _lo for q = xbar, cmf, cfb, M0, weight (every slice), G (the fixture's
                          G_slices), M00, energy, nav; b6_wx, b6_rx (weights after every slice [2 L, nw], rows [3, 10])
                          and b6_parents of the driver run, fields and comb uniforms replayed from the seed
  thermal_hubbard_cont_far_ext.npz
                          h10_<q> of the case a10 (8 x 16), G_last in place of G; hb3_wx, hb3_rx, hb3_parents of the
                          driver run b3 (10 x 10)
  thermal_far_bins_ext.npz
                          a8_right, a8_bin, h10_right, h10_bin: what the slice kernels write behind the slices
                          BIN_SLICES of tests/thermal_far_cases.py, the rows bin_rows(M)
<q>_hi + <q>_lo is the extended number (tests/thermal_wide_cases.py: split, joined).  Needs no reference: it reads the
fixtures only for the parameters and the fields of the cases.  tests/test_thermal_far_cpu.py recomputes the first slice
of both single-walker cases and compares it with what is stored here.

Usage:  python tests/golden/make_thermal_far_ext.py [ueg|hubbard|bins]            (writes the files under tests/golden/)
        python tests/golden/make_thermal_far_ext.py [ueg|hubbard|bins] --check    recompute and compare with the committed files
"""
import os
import sys

import numpy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import thermal_far_cases as F                                  # noqa: E402
from tests import thermal_wide_cases as W                                 # noqa: E402
from tests.golden.make_thermal_ueg_paths_ext import run_case              # noqa: E402
from tests.golden.make_thermal_wide_ext import put                        # noqa: E402

MAX_BYTES = 1024 * 1024                   # of a committed file


def make_ueg():
    out = {}
    put(out, F.UEG_A, W.ueg_run(F.UEG, F.UEG_A, True))
    pre = 'b%d_' % F.UEG_B
    b = run_case(W.golden(F.UEG), F.UEG_B, kits=('ext',))
    for key in ('wx_hi', 'wx_lo', 'rx_hi', 'rx_lo', 'parents'):
        out[pre + key] = b[pre + key]
    return out


def make_hubbard():
    out = {}
    put(out, 'h%d_' % F.HUBBARD_A, F.hubbard_run(True))
    rows, wts, parents, _ = F.hubbard_driver(True)
    pre = 'hb%d_' % F.HUBBARD_B
    out[pre + 'wx_hi'], out[pre + 'wx_lo'] = W.split(wts)
    out[pre + 'rx_hi'], out[pre + 'rx_lo'] = W.split(rows)
    out[pre + 'parents'] = numpy.array(parents)
    return out


def make_bins():
    out = {}
    for which, pre in (('ueg', F.UEG_A), ('hubbard', 'h%d_' % F.HUBBARD_A)):
        for q, v in F.bins_run(which, True).items():
            out[pre + q + '_hi'], out[pre + q + '_lo'] = W.split(v, small=True)
    return out


if __name__ == '__main__':
    which = [a for a in sys.argv[1:] if not a.startswith('--')] or ['ueg', 'hubbard', 'bins']
    status = 0
    for w in which:
        name = F.BINS_EXT if w == 'bins' else F.EXT_OF[F.UEG if w == 'ueg' else F.HUBBARD]
        out = make_bins() if w == 'bins' else make_ueg() if w == 'ueg' else make_hubbard()
        path = os.path.join(HERE, name)
        if '--check' in sys.argv[1:]:
            old = numpy.load(path)
            bad = [key for key, v in out.items() if not numpy.array_equal(old[key], v)]
            print('%s %s' % (name, 'reproduces' if not bad else 'DIFFERS: ' + ', '.join(bad)))
            status |= 1 if bad else 0
        else:
            numpy.savez_compressed(path, **out)
            assert os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
            print('%s %d bytes' % (name, os.path.getsize(path)))
    sys.exit(status)
