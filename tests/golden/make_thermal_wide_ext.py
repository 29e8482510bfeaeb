#!/usr/bin/env python3
"""The cases of the wide fixtures (thermal_ueg81.npz, thermal_ueg93.npz, thermal_hubbard_cont_wide.npz) through the
extended-precision restatements of the tests, stored so that the GPU tests can hold them to the accuracy rule without
running numpy.clongdouble themselves (one slice at M = 93 takes seconds, the driver at M = 81 minutes).  One file per
fixture, each below the size of a committed file:

  thermal_ueg81_ext.npz   a6_<q>_hi / _lo for q = xbar, cmf, cfb, M0, weight (every slice), G (the fixture's
                          G_slices), M00, energy, nav; b5_wx, b5_rx (weights after every slice [2 L, nw], rows [3, 10])
                          and b5_parents of the driver run, fields and comb uniforms replayed from the seed
  thermal_ueg93_ext.npz   a7_<q>_hi / _lo likewise
  thermal_hubbard_cont_wide_ext.npz
                          h8_<q>, h9_<q> of the cases a8 (8 x 8) and a9 (1 x 65), G_last in place of G; hb2_wx, hb2_rx,
                          hb2_parents of the driver run b2
<q>_hi + <q>_lo is the extended number (tests/thermal_wide_cases.py: split, joined).  Needs no reference: it reads the
fixtures only for the parameters and the fields of the cases.  tests/test_thermal_wide_cpu.py recomputes the first
slices of every single-walker case and compares them with what is stored here.

Usage:  python tests/golden/make_thermal_wide_ext.py            (writes the three files under tests/golden/)
        python tests/golden/make_thermal_wide_ext.py --check    recompute and compare with the committed files
"""
import os
import sys

import numpy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import thermal_wide_cases as W                                 # noqa: E402
from tests.golden.make_thermal_ueg_paths_ext import run_case              # noqa: E402

MAX_BYTES = 1024 * 1024                   # of a committed file
BIG = ('G', 'G_last')                     # stored with a single-precision remainder


def put(out, pre, run):
    for q, v in run.items():
        if q in ('nclip', 'min_cos_margin'):
            continue
        out[pre + q + '_hi'], out[pre + q + '_lo'] = W.split(v, small=q in BIG)
    assert run['min_cos_margin'] > 1e-6, (pre, run['min_cos_margin'])


def make():
    files = {}
    for name, pre in W.UEG_A:
        out = files.setdefault(W.EXT_OF[name], {})
        put(out, pre, W.ueg_run(name, pre, True))
    name, k = W.UEG_B
    b = run_case(W.golden(name), k, kits=('ext',))
    pre = 'b%d_' % k
    out = files[W.EXT_OF[name]]
    out[pre + 'wx_hi'], out[pre + 'wx_lo'] = b[pre + 'wx_hi'], b[pre + 'wx_lo']
    out[pre + 'rx_hi'], out[pre + 'rx_lo'] = b[pre + 'rx_hi'], b[pre + 'rx_lo']
    out[pre + 'parents'] = b[pre + 'parents']
    out = files.setdefault(W.EXT_OF[W.HUBBARD], {})
    for k in W.HUBBARD_A:
        put(out, 'h%d_' % k, W.hubbard_run(k, True))
    rows, wts, parents, _ = W.hubbard_driver(True)
    pre = 'hb%d_' % W.HUBBARD_B
    out[pre + 'wx_hi'], out[pre + 'wx_lo'] = W.split(wts)
    out[pre + 'rx_hi'], out[pre + 'rx_lo'] = W.split(rows)
    out[pre + 'parents'] = numpy.array(parents)
    return files


if __name__ == '__main__':
    files = make()
    status = 0
    for name, out in files.items():
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
