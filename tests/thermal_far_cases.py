"""What the CPU and the GPU tests of the far route (AFQ_THERMAL_FAR) share: the two fixtures recorded from the
reference where only that route runs (tests/golden/thermal_ueg123.npz: the shell of 123 plane waves;
thermal_hubbard_cont_far.npz: 8 x 16, M = 128, and the driver on 10 x 10), the restatements run over a fixture case in
either kit, and their stored extended-precision results (thermal_ueg123_ext.npz, thermal_hubbard_cont_far_ext.npz,
written by tests/golden/make_thermal_far_ext.py).  The layout and the helpers are those of tests/thermal_wide_cases.py;
the Hubbard case keeps one spin of dmat, dmat_inv and BH1 (both spins are equal), which hubbard_constants gives back as
[2, M, M]."""
import numpy

from tests import thermal_hubbard_cont_ref as R
from tests import thermal_wide_cases as W
from tests.thermal_ueg_ref import Kit64
from tests.thermal_ueg_ref_ext import KitExt

UEG = "thermal_ueg123.npz"
UEG_A, UEG_B = "a8_", 6
HUBBARD = "thermal_hubbard_cont_far.npz"
HUBBARD_A, HUBBARD_B = 10, 3
EXT_OF = {UEG: "thermal_ueg123_ext.npz", HUBBARD: "thermal_hubbard_cont_far_ext.npz"}
# What the slice kernels write, `right` and the bin of the slice's block, of the two single-walker cases in extended
# precision: behind the slices BIN_SLICES (counted from 1: the second of bin 0, the first of bin 1, the last) and for
# the rows bin_rows(M) (every 16th and the last: the whole matrices would be beyond the size of a committed file)
BINS_EXT = "thermal_far_bins_ext.npz"
BIN_SLICES = (2, 6, 10)


def bin_rows(M):
    return numpy.array(sorted(set(range(0, M, 16)) | {M - 1}))


golden, split, joined = W.golden, W.split, W.joined


def stored_ext():
    out = {}
    for name in list(EXT_OF.values()) + [BINS_EXT]:
        out.update(golden(name))
    return out


def hubbard_constants(d, pre):
    """(dmat, dmat_inv, BH1) [2, M, M] of a case that stores one spin."""
    return tuple(numpy.ascontiguousarray(numpy.repeat(d[pre + q], 2, axis=0)) for q in ('dmat', 'dmat_inv', 'BH1'))


def hubbard_path(d, pre, ext, nw=1):
    system = W.hubbard_system(d, pre)
    L = int(round(float(d[pre + 'beta']) / float(d[pre + 'dt'])))
    dmat, dmat_inv, BH1 = hubbard_constants(d, pre)
    return R.Path(system.H1, float(d[pre + 'U']), dmat, dmat_inv, BH1, d[pre + 'mf_shift'], complex(d[pre + 'mf_const_fac']),
                  float(d[pre + 'dt']), L, int(d[pre + 'stack_size']), nw, kit=KitExt if ext else Kit64)


def hubbard_device(d, pre, nw, options):
    from tests.thermal_hubbard_cont_cases import device_of
    L = int(round(float(d[pre + 'beta']) / float(d[pre + 'dt'])))
    dmat, dmat_inv, BH1 = hubbard_constants(d, pre)
    return device_of(W.hubbard_system(d, pre), dmat, dmat_inv, BH1, d[pre + 'mf_shift'], complex(d[pre + 'mf_const_fac']),
                     float(d[pre + 'dt']), L, int(d[pre + 'stack_size']), nw, options)


def hubbard_run(ext, nslice=None):
    """Case a10 slice by slice through the restatement, as W.hubbard_run."""
    d = golden(HUBBARD)
    pre = 'a%d_' % HUBBARD_A
    p = hubbard_path(d, pre, ext)
    out = {n: [] for n in W.SCALARS}
    out['M00'] = p.M0[0].copy()
    for ts in range(p.L if nslice is None else nslice):
        xbar, cmf, cfb = p.step(d[pre + 'xi'][ts][None])
        out['xbar'].append(xbar[0]); out['cmf'].append(cmf[0]); out['cfb'].append(cfb[0])
        out['M0'].append(p.M0[0].copy()); out['weight'].append(p.weight[0])
    E, nav = p.energy()
    out.update(G_last=p.G[0].copy(), energy=E[0], nav=nav[0], nclip=p.nclip, min_cos_margin=p.min_cos_margin)
    return {n: numpy.array(v) if isinstance(v, list) else v for n, v in out.items()}


def hubbard_driver(ext):
    """Driver run b3 through the restatement -> (rows [3, 10], weights [2 L, nw], parents, path)."""
    from pauxy_amd.trial_density import OneBody
    d = golden(HUBBARD)
    pre = 'b%d_' % HUBBARD_B
    system = W.hubbard_system(d, pre)
    dt = float(d[pre + 'dt'])
    trial = OneBody(system, float(d[pre + 'beta']), dt)
    BH1, mf_shift, _, mfc = R.constants(system.T[0], system.U, system.mu, dt, numpy.asarray(trial.dmat.real))
    xis, us = W.hubbard_driver_fields(d, pre)
    p = R.Path(system.H1, system.U, trial.dmat.real, trial.dmat_inv.real, BH1, mf_shift, mfc, dt, int(d[pre + 'ntime_slices']),
               int(d[pre + 'stack_size']), int(d[pre + 'nwalkers']), kit=KitExt if ext else Kit64)
    rows, wts, parents = p.run(xis, us, 2, int(d[pre + 'npop_control']))
    return rows, wts, parents, p


def case_path(which, ext):
    """(fixture, prefix, the restatement's Path of one walker) of the single-walker case: 'ueg' (a8) or 'hubbard' (a10)."""
    if which == 'ueg':
        d = golden(UEG)
        c = W.case_of_fixture(d, UEG_A)
        ss = int(d[UEG_A + 'stack_size'])
        return d, UEG_A, (c.path_ext(ss, 1) if ext else c.path64(ss, 1))
    d = golden(HUBBARD)
    pre = 'a%d_' % HUBBARD_A
    return d, pre, hubbard_path(d, pre, ext)


def bins_run(which, ext, upto=None):
    """`right` [len(BIN_SLICES), 2, rows, M] and the bin the slice wrote, likewise, of the single-walker case; upto: the
    slices to that one only."""
    d, pre, p = case_path(which, ext)
    rows = bin_rows(p.M)
    right, bins = [], []
    for ts in range(max(BIN_SLICES) if upto is None else upto):
        block = ts // p.stack_size
        p.step(d[pre + 'xi'][ts][None])
        if ts + 1 in BIN_SLICES:
            right.append(p.right[0][:, rows].copy())
            bins.append(p.stack[0, block][:, rows].copy())
    return {'right': numpy.array(right), 'bin': numpy.array(bins)}
