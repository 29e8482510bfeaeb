"""Inputs shared by the tests of the delayed-update route of the real thermal walkers (AFQ_THERMAL_DELAYED,
walkers: {delayed_updates: True}), and the numpy restatement of the delayed site loop, which is the specification of
thermal_slice_delayed_kernel:

  for every panel of KB sites i0 .. i0 + kb - 1 (the last one ragged):
    Cp = G[:, i0 : i0 + kb], Rp = G[i0 : i0 + kb, :] (per spin) are copied out and kept current;
    site i = i0 + j: g = Cp[i, j] of both spins gives the two probabilities, the uniform is consumed, the weight
      takes norm exp(eshift) and the field is u < p_0 / norm as in thermal_ref.Path.sites;
      u = -f Cp[:, j], w = e_i - Rp[j, :] (both zero where the norm vanished: weight 0, field -1, BV = auxf[0]);
      Cp[:, j + 1 :] += u w[i0 + j + 1 : i0 + kb] and Rp[j + 1 :, :] += u[i0 + j + 1 : i0 + kb] w;
      U[:, j] = u, W[j, :] = w;
    G <- G + U W.

DelayedPath is thermal_ref.Path with that site loop, in the number type of its kit (fp64, or thermal_ref_ext's)."""
import numpy

from tests import thermal_ref as tr
from tests import thermal_ref_ext as te
from tests.thermal_cases import Case

KB = 16                         # the kernel's panel (TD_KB of k_thermal.hip)
DELAYED_MAX = 128               # afq_thermal_delayed_max_basis(): the 128 columns of two per lane
LDS_MAX = 160 * 1024


def greens_wide_lds(M):
    """ts_greens_wide_lds<double>: one matrix of pitch M | 1 and 1152 scalars of vectors, 128 ints."""
    return 8 * (M * (M | 1) + 1152) + 512


def slice_delayed_lds(M):
    """th_slice_delayed_lds: bv [2][128]; the larger of the panels (columns and U of pitch KB + 1, rows and W of pitch
    M | 1, both spins) and the stack update's one matrix."""
    panels = 2 * (2 * M * (KB + 1) + 2 * KB * (M | 1))
    return 8 * (256 + max(panels, M * (M | 1)))


def wrap_lds(M):
    return 8 * M * (M | 1)


def bound_by_formula():
    m = 128
    while m > 1 and max(greens_wide_lds(m), slice_delayed_lds(m), wrap_lds(m)) > LDS_MAX:
        m -= 1
    return m


class DelayedPath(tr.Path):
    """thermal_ref.Path whose M single-site updates run as delayed updates in panels of `kb_max` sites."""

    def __init__(self, *args, **kw):
        self.kb_max = kw.pop('KB', KB)
        tr.Path.__init__(self, *args, **kw)

    def sites(self, u, eshift=0.0):
        dt = self.kit.dtype
        nw, M = self.nw, self.M
        u = numpy.asarray(u, dtype=dt)
        delta = self.auxf - 1
        fields = numpy.full((nw, M), -1, dtype=numpy.int32)
        BV = numpy.broadcast_to(self.auxf[0][None, :, None], (nw, 2, M)).copy()
        G = self.G
        ex = numpy.exp(dt(eshift))
        for i0 in range(0, M, self.kb_max):
            kb = min(self.kb_max, M - i0)
            Cp = G[:, :, :, i0:i0 + kb].copy()
            Rp = G[:, :, i0:i0 + kb, :].copy()
            Uf = numpy.zeros((nw, 2, M, kb), dtype=dt)
            Wf = numpy.zeros((nw, 2, kb, M), dtype=dt)
            for j in range(kb):
                i = i0 + j
                g = Cp[:, :, i, j]                                                   # [nw, spin]
                probs = dt(0.5) * numpy.prod(1 + (1 - g)[:, None, :] * delta[None, :, :], axis=2)
                p = numpy.maximum(probs, 0)
                norm = p[:, 0] + p[:, 1]
                ok = norm > 0
                safe = numpy.where(ok, norm, 1)
                self.weight = numpy.where(ok, self.weight * norm * ex, 0)
                thr = p[:, 0] / safe
                x = numpy.where(u[:, i] < thr, 0, 1)
                if ok.any():
                    self.min_margin = min(self.min_margin, float(numpy.min(numpy.abs(u[:, i] - thr)[ok])))
                d = delta[x]
                f = d / (1 + (1 - g) * d)
                uv = numpy.where(ok[:, None, None], -f[:, :, None] * Cp[:, :, :, j], 0)    # [nw, spin, M]
                wv = -Rp[:, :, j, :]
                wv[:, :, i] += 1
                wv = numpy.where(ok[:, None, None], wv, 0)
                Cp[:, :, :, j + 1:] += uv[:, :, :, None] * wv[:, :, None, i + 1:i0 + kb]
                Rp[:, :, j + 1:, :] += uv[:, :, i + 1:i0 + kb, None] * wv[:, :, None, :]
                Uf[:, :, :, j] = uv
                Wf[:, :, j, :] = wv
                BV[ok, :, i] = self.auxf[x[ok]]
                fields[ok, i] = x[ok]
            G = G + Uf @ Wf
        self.G = G
        return fields, BV


def paths(case, Lts, stack_size, nstblz, nw, kb=KB):
    """(fp64 delayed restatement, extended direct restatement) of one case."""
    args = (case.BT, case.BH1, case.auxf, Lts, stack_size, nstblz, nw)
    p64 = DelayedPath(*args, BT_inv=case.BT_inv, KB=kb)
    px = te.path(*args, BT_inv=case.BT_inv)
    return p64, px


def delayed_device(case, nw, Lts, stack_size, nstblz, options=0):
    from pauxy_amd import _lib as L
    return case.device(nw, Lts, stack_size, nstblz, options=L.THERMAL_DELAYED | options)


class FixtureCase(object):
    """A recorded lattice (cases c, d of thermal_hubbard_large*.npz) with the members of thermal_cases.Case that the
    tests read: a matrix the maker found rebuilt to the bit by tests/thermal_ref is rebuilt here, the others are the
    stored ones."""

    def __init__(self, d, tag):
        self.nx, self.ny = int(d[tag + '_nx']), int(d[tag + '_ny'])
        self.M = self.nx * self.ny
        self.U, self.dt = float(d[tag + '_U']), float(d[tag + '_dt'])
        self.mu, self.mu_trial = float(d[tag + '_mu_system']), float(d[tag + '_mu'])
        T = tr.hubbard_kinetic(self.nx, self.ny)
        H1 = numpy.array([T, T])
        BT, BT_inv = tr.one_body_dmat(H1, self.mu_trial, self.dt)
        mine = {'T': H1, 'dmat': BT, 'dmat_inv': BT_inv, 'BH1': BT,
                'auxf': tr.hubbard_auxf(self.U, self.dt, self.mu, self.mu_trial)}
        m = {}
        for name, same in zip(d[tag + '_rebuilt_names'], d[tag + '_rebuilt']):
            assert bool(same) != (tag + '_' + str(name) in d)
            m[str(name)] = mine[str(name)] if bool(same) else d[tag + '_' + str(name)]
        self.H1, self.BT, self.BT_inv, self.BH1, self.auxf = m['T'], m['dmat'], m['dmat_inv'], m['BH1'], m['auxf']
        self.na, self.nb = [int(x) for x in d[tag + '_nelec']]
        self.L, self.stack_size, self.nstblz = int(d[tag + '_num_slices']), int(d[tag + '_stack_size']), int(d[tag + '_nstblz'])

    device = Case.device
    h1_scale = Case.h1_scale

    def args(self, nw=1):
        return (self.BT, self.BH1, self.auxf, self.L, self.stack_size, self.nstblz, nw)
