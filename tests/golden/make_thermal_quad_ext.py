#!/usr/bin/env python3
"""The cases of the quad fixtures (thermal_ueg147.npz, thermal_hubbard_cont_quad.npz) through the extended-precision
restatements of the tests, and the Green's function alone where only the quad route runs, stored so that the GPU tests
can hold them to the accuracy rule without running numpy.clongdouble themselves, as make_thermal_far_ext.py does for the
far fixtures (whose helpers this imports).  One file per part, each below the size of a committed file:

  thermal_ueg147_ext.npz  a9_<q>_hi / _lo for q = xbar, cmf, cfb, M0, weight (every slice), G (the fixture's
                          G_slices, the rows a9_G_rows = Q.ueg_g_rows(147)), M00, energy, nav; b7_wx, b7_rx (weights after every slice [2 L, nw], rows [3, 10])
                          and b7_parents of the driver run, fields and comb uniforms replayed from the seed
  thermal_hubbard_cont_quad_ext.npz
                          h11_<q> of the case a11 (16 x 16): the scalars of every slice, M00, energy, nav, and the rows
                          a11_rows of G_last, bins_last and right_last; hb4_wx, hb4_rx, hb4_parents of the driver run
                          b4 (12 x 12)
  thermal_quad_greens_ext.npz
                          for every (M, bins) of tests/thermal_quad_cases.py GREENS_CASES: g<M>_<bins>_G_hi / _lo, the
                          rows rows_of(M) of G [2, rows, M] of one walker at slice_ix 0, g.._det_hi / _lo [2], and
                          g.._G_err64, g.._det_err64: the distance of the fp64 restatement from the extended result
                          (G on the scale max(1, max |G|), det relative), which is err_ref of the rule where no
                          reference run exists
<q>_hi + <q>_lo is the extended number (tests/thermal_wide_cases.py: split, joined).  Needs no reference: it reads the
fixtures only for the parameters and the fields of the cases.  tests/test_thermal_quad_cpu.py recomputes parts of it.

Usage:  python tests/golden/make_thermal_quad_ext.py [ueg|hubbard|greens]            (writes the files under tests/golden/)
        python tests/golden/make_thermal_quad_ext.py [ueg|hubbard|greens] --check    recompute and compare with the committed files
"""
import os
import sys

import numpy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import thermal_quad_cases as Q                                 # noqa: E402
from tests import thermal_wide_cases as W                                 # noqa: E402
from tests.golden.make_thermal_far_ext import MAX_BYTES                   # noqa: E402
from tests.golden.make_thermal_ueg_paths_ext import run_case              # noqa: E402
from tests.golden.make_thermal_wide_ext import put                        # noqa: E402

BIG = ('G_last', 'bins_last', 'right_last')


def make_ueg():
    out = {}
    run = W.ueg_run(Q.UEG, Q.UEG_A, True)
    rows = Q.ueg_g_rows(run['G'].shape[-1])
    run['G'] = run['G'][:, :, rows]
    put(out, Q.UEG_A, run)
    out[Q.UEG_A + 'G_rows'] = rows
    pre = 'b%d_' % Q.UEG_B
    b = run_case(W.golden(Q.UEG), Q.UEG_B, kits=('ext',))
    for key in ('wx_hi', 'wx_lo', 'rx_hi', 'rx_lo', 'parents'):
        out[pre + key] = b[pre + key]
    return out


def make_hubbard():
    out = {}
    run = Q.hubbard_run(True)
    pre = 'h%d_' % Q.HUBBARD_A
    put(out, pre, {q: v for q, v in run.items() if q not in BIG})
    for q in BIG:
        out[pre + q + '_hi'], out[pre + q + '_lo'] = W.split(run[q], small=True)
    rows, wts, parents, _ = Q.hubbard_driver(True)
    pre = 'hb%d_' % Q.HUBBARD_B
    out[pre + 'wx_hi'], out[pre + 'wx_lo'] = W.split(wts)
    out[pre + 'rx_hi'], out[pre + 'rx_lo'] = W.split(rows)
    out[pre + 'parents'] = numpy.array(parents)
    return out


def make_greens():
    out = {}
    for M, nbins in Q.GREENS_CASES:
        key = Q.greens_key(M, nbins)
        Gx, detx = Q.greens_run(M, nbins, True)
        G64, det64 = Q.greens_run(M, nbins, False)
        out[key + 'G_hi'], out[key + 'G_lo'] = W.split(Gx, small=True)
        out[key + 'det_hi'], out[key + 'det_lo'] = W.split(detx)
        out[key + 'G_err64'] = numpy.float64(Q.err_of(G64, Gx))
        out[key + 'det_err64'] = numpy.float64(Q.err_of(det64, detx, relative=True))
        out[key + 'rows'] = Q.rows_of(M)
        print('%s G err64 %.3e det err64 %.3e' % (key, out[key + 'G_err64'], out[key + 'det_err64']), flush=True)
    return out


if __name__ == '__main__':
    which = [a for a in sys.argv[1:] if not a.startswith('--')] or ['ueg', 'hubbard', 'greens']
    status = 0
    for w in which:
        name = Q.GREENS_EXT if w == 'greens' else Q.EXT_OF[Q.UEG if w == 'ueg' else Q.HUBBARD]
        out = make_greens() if w == 'greens' else make_ueg() if w == 'ueg' else make_hubbard()
        path = os.path.join(HERE, name)
        if '--check' in sys.argv[1:]:
            old = numpy.load(path)
            # (the distances of the fp64 restatement go through LAPACK: they are compared in magnitude)
            bad = [key for key, v in out.items()
                   if not (numpy.allclose(old[key], v, rtol=0.5, atol=0) if key.endswith('err64') else numpy.array_equal(old[key], v))]
            print('%s %s' % (name, 'reproduces' if not bad else 'DIFFERS: ' + ', '.join(bad)))
            status |= 1 if bad else 0
        else:
            numpy.savez_compressed(path, **out)
            assert os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
            print('%s %d bytes' % (name, os.path.getsize(path)))
    sys.exit(status)
