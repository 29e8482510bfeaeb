"""What the CPU and the GPU tests of the quad route (AFQ_THERMAL_QUAD, walkers: {quad_basis: True}) share: the two
fixtures recorded from the reference where only that route runs (tests/golden/thermal_ueg147.npz: the shell of 147 plane
waves; thermal_hubbard_cont_quad.npz: 16 x 16, M = 256, and the driver on 12 x 12), the restatements run over a fixture
case in either kit, their stored extended-precision results (thermal_ueg147_ext.npz, thermal_hubbard_cont_quad_ext.npz)
and the Green's functions alone at M = 129, 193 and 256 (thermal_quad_greens_ext.npz), all three written by
tests/golden/make_thermal_quad_ext.py.  The layout and the helpers are those of tests/thermal_far_cases.py.

A [2, 256, 256] complex matrix is 2 MiB, so above M = 147 matrices are stored and compared on the rows rows_of(M): the
ends of the four column classes of a lane (0, 63 | 64, 127 | 128, 191 | 192, 255) that M holds, and the last row.  A row
crosses every column class."""
import numpy

from tests import thermal_far_cases as F
from tests import thermal_hubbard_cont_ref as R
from tests import thermal_ueg_ref as ur
from tests import thermal_ueg_ref_ext as ue
from tests import thermal_wide_cases as W
from tests.thermal_ueg_ref import Kit64
from tests.thermal_ueg_ref_ext import KitExt

UEG = "thermal_ueg147.npz"
UEG_A, UEG_B = "a9_", 7
HUBBARD = "thermal_hubbard_cont_quad.npz"
HUBBARD_A, HUBBARD_B = 11, 4
EXT_OF = {UEG: "thermal_ueg147_ext.npz", HUBBARD: "thermal_hubbard_cont_quad_ext.npz"}
GREENS_EXT = "thermal_quad_greens_ext.npz"
# The Green's function alone where only the quad route runs: (M, bins) -- 129: one column in the third class of a lane;
# 193: one in the fourth; 256: all four full -- one walker, bins of 2 slices built as every thermal test builds them
# (thermal_ueg_cases.Case.random_stack, seed 5), the chain of slice_ix 0
GREENS_CASES = ((129, 2), (129, 5), (193, 2), (193, 5), (256, 2), (256, 5))
GREENS_SEED, GREENS_STACK_SIZE = 5, 2

golden, split, joined = W.golden, W.split, W.joined


def rows_of(M):
    return numpy.array(sorted({r for r in (0, 63, 64, 127, 128, 191, 192) if r < M} | {M - 1}))


def ueg_g_rows(M):
    """The rows of the M = 147 Green's function the extended file holds (hi and lo of all 147 would be beyond the size of
    a committed file): every second row, and rows_of(M)."""
    return numpy.array(sorted(set(range(0, M, 2)) | set(rows_of(M).tolist())))


def stored_ext():
    out = {}
    for name in list(EXT_OF.values()) + [GREENS_EXT]:
        out.update(golden(name))
    return out


# ---- the Green's function alone
def greens_stack(M, nbins):
    """c128 [1, nbins, 2, M, M]: what the device is given."""
    from tests.test_gpu_thermal_wide import complex_stack
    return complex_stack(M, 1, nbins, GREENS_STACK_SIZE, GREENS_SEED)


def greens_key(M, nbins):
    return 'g%d_%d_' % (M, nbins)


def greens_run(M, nbins, ext):
    """(G [2, rows_of(M), M], det [2]) of the chain of slice_ix 0 through the restatement in either kit."""
    stack = greens_stack(M, nbins)
    bins = [stack[:, b].reshape(2, M, M) for b in ur.chain_order(0, GREENS_STACK_SIZE, nbins)]
    kit = KitExt if ext else Kit64
    G = kit.strat_greens(bins)
    return G[:, rows_of(M)], kit.det(G)


# ---- the Hubbard cases
def hubbard_device(nw, options):
    return F.hubbard_device(golden(HUBBARD), 'a%d_' % HUBBARD_A, nw, options)


def hubbard_run(ext, nslice=None):
    """Case a11 (16 x 16) slice by slice through the restatement, as F.hubbard_run; behind the last slice the rows
    rows_of(M) of G, of every bin and of right."""
    d = golden(HUBBARD)
    pre = 'a%d_' % HUBBARD_A
    p = F.hubbard_path(d, pre, ext)
    rows = d[pre + 'rows']
    out = {n: [] for n in W.SCALARS}
    out['M00'] = p.M0[0].copy()
    for ts in range(p.L if nslice is None else nslice):
        xbar, cmf, cfb = p.step(d[pre + 'xi'][ts][None])
        out['xbar'].append(xbar[0]); out['cmf'].append(cmf[0]); out['cfb'].append(cfb[0])
        out['M0'].append(p.M0[0].copy()); out['weight'].append(p.weight[0])
    E, nav = p.energy()
    out.update(G_last=p.G[0][:, rows].copy(), bins_last=p.stack[0][:, :, rows].copy(), right_last=p.right[0][:, rows].copy(),
               energy=E[0], nav=nav[0], nclip=p.nclip, min_cos_margin=p.min_cos_margin)
    return {n: numpy.array(v) if isinstance(v, list) else v for n, v in out.items()}


def hubbard_driver(ext):
    """Driver run b4 (12 x 12) through the restatement -> (rows [3, 10], weights [2 L, nw], parents, path)."""
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


def err_of(got, want_ext, relative=False):
    """The distance the rule is stated in: relative for determinants and weights, else on the scale max(1, max |want|)."""
    return ue.rerr(got, want_ext) if relative else ue.gerr(got, want_ext)
