"""Thin numpy-facing wrapper over the C ABI: one ``AfqDevice`` per GPU.

Every array crossing this boundary is a C-contiguous numpy array; complex128
arrays are passed as their interleaved (re, im) storage, exactly what
``include/afqmc_hip.h`` documents.  All arithmetic happens in the library.
"""
import ctypes

import numpy

from pauxy_amd import _lib as L


def _c128(a, shape=None):
    a = numpy.ascontiguousarray(a, dtype=numpy.complex128)
    if shape is not None:
        assert a.shape == tuple(shape), (a.shape, shape)
    return a


def _f64(a, shape=None):
    a = numpy.ascontiguousarray(a, dtype=numpy.float64)
    if shape is not None:
        assert a.shape == tuple(shape), (a.shape, shape)
    return a


def _i64(a):
    return numpy.ascontiguousarray(a, dtype=numpy.int64)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _flatten_ragged(lists):
    off = numpy.zeros(len(lists) + 1, dtype=numpy.int64)
    off[1:] = numpy.cumsum([len(x) for x in lists])
    flat = numpy.concatenate([numpy.asarray(x, dtype=numpy.int64) for x in lists]) if off[-1] else \
        numpy.zeros(0, dtype=numpy.int64)
    return off, _i64(flat)


class AfqDevice(object):
    def __init__(self, device_id=0):
        self.lib = L.load()
        self.h = ctypes.c_void_p()
        rc = self.lib.afq_create(int(device_id), ctypes.byref(self.h))
        if rc != 0:
            raise L.AfqError(rc, "afq_create failed (no usable MI355X device %d?)" % device_id)
        self.device_id = device_id
        self.kind = None
        self.nw = 0

    # -- plumbing ---------------------------------------------------------
    def _ck(self, rc):
        if rc != 0:
            raise L.AfqError(rc, self.lib.afq_last_error(self.h).decode())

    def close(self):
        if self.h:
            self.lib.afq_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._ck(self.lib.afq_sync(self.h))

    # -- inputs -----------------------------------------------------------
    def set_system_generic(self, hs_pot, rchol, H1, ecore, na, nb):
        H1 = _c128(H1)
        M = H1.shape[-1]
        # complex Cholesky vectors with an imaginary part go to the c128 entry point; everything else
        # takes the real one unchanged
        cplx = numpy.iscomplexobj(hs_pot) and bool(numpy.any(numpy.asarray(hs_pot).imag != 0))
        hs_pot = _c128(hs_pot) if cplx else _f64(hs_pot)
        K = hs_pot.shape[1]
        assert hs_pot.shape == (M * M, K)
        rchol = _c128(rchol, ((na + nb) * M, K))
        fn = self.lib.afq_set_system_generic_c128 if cplx else self.lib.afq_set_system_generic
        self._ck(fn(self.h, M, K, na, nb, _p(hs_pot), _p(rchol), _p(H1), float(numpy.real(ecore))))
        self.kind, self.M, self.K, self.na, self.nb = 'generic', M, K, na, nb

    def set_system_hubbard(self, T, U, na, nb):
        T = _c128(T)
        M = T.shape[-1]
        self._ck(self.lib.afq_set_system_hubbard(self.h, M, na, nb, float(U), _p(T)))
        self.kind, self.M, self.K, self.na, self.nb = 'hubbard', M, M, na, nb

    def set_system_ueg(self, iA, iB, ikpq_i, ikpq_kpq, ipmq_i, ipmq_pmq, vqvec, vol, H1diag, ecore, na, nb):
        iA = iA.tocsc()
        iB = iB.tocsc()
        iA.sort_indices()
        iB.sort_indices()
        H1diag = _f64(H1diag)
        M = H1diag.shape[-1]
        nq = iA.shape[1]
        koff, ki = _flatten_ragged(ikpq_i)
        _, kk = _flatten_ragged(ikpq_kpq)
        poff, pi = _flatten_ragged(ipmq_i)
        _, pp = _flatten_ragged(ipmq_pmq)
        arrs = [_i64(iA.indptr), _i64(iA.indices), _c128(iA.data), _i64(iB.indptr), _i64(iB.indices),
                _c128(iB.data), koff, ki, kk, poff, pi, pp, _f64(vqvec)]
        self._ck(self.lib.afq_set_system_ueg(self.h, M, nq, na, nb, *[_p(a) for a in arrs], float(vol),
                                             _p(H1diag), float(ecore)))
        self.kind, self.M, self.K, self.na, self.nb = 'ueg', M, 2 * nq, na, nb
        self.nq = nq

    def set_trial(self, psi):
        self.ndet = 1
        psi = _c128(psi, (self.M, self.na + self.nb))
        self._ck(self.lib.afq_set_trial(self.h, _p(psi)))

    def inverse_overlap(self):
        """(O^-1 [nw, 2, nmax, nmax], overlap [nw]) with O = phi_s^T conj(psi_s)."""
        nmax = max(self.na, self.nb)
        out = numpy.zeros((self.nw, 2, nmax, nmax), dtype=numpy.complex128)
        ov = numpy.zeros(self.nw, dtype=numpy.complex128)
        self._ck(self.lib.afq_inverse_overlap(self.h, _p(out), _p(ov)))
        return out, ov

    # ---- discrete Hirsch propagator
    def set_propagator_hirsch(self, bt2, dt, charge_decomposition=False):
        bt2 = _c128(bt2, (2, self.M, self.M))
        self._ck(self.lib.afq_set_propagator_hirsch(self.h, _p(bt2), float(dt), int(bool(charge_decomposition))))
        self.nv = 1

    def propagate_hirsch(self, eshift):
        self._ck(self.lib.afq_propagate_hirsch(self.h, float(numpy.real(eshift))))

    def hirsch_single_site(self, on=True):
        """on=False: two_body_direct (propagation/hubbard.py:222-275) instead of the M single-site updates."""
        self._ck(self.lib.afq_hirsch_single_site(self.h, 1 if on else 0))

    def hirsch_free_projection(self, on=True):
        self._ck(self.lib.afq_hirsch_free_projection(self.h, 1 if on else 0))

    def propagate_hirsch_free(self, u, eshift, fetch_fields=False):
        """propagation/hubbard.py:303-343 for every walker with |weight| > 1e-8; u [nw, M] or None (device stream)."""
        u_ = None if u is None else _f64(u, (self.nw, self.M))
        fields = numpy.zeros((self.nw, self.M), dtype=numpy.int32) if fetch_fields else None
        self._ck(self.lib.afq_propagate_hirsch_free(self.h, _p(u_), _p(fields), float(eshift)))
        return fields

    def hirsch_kinetic(self):
        self._ck(self.lib.afq_hirsch_kinetic(self.h))

    def hirsch_two_body(self, u):
        u = numpy.ascontiguousarray(u, dtype=numpy.float64).reshape(self.nw, self.M)
        fields = numpy.zeros((self.nw, self.M), dtype=numpy.int32)
        used = numpy.zeros(self.nw, dtype=numpy.int32)
        self._ck(self.lib.afq_hirsch_two_body(self.h, _p(u), _p(fields), _p(used)))
        return fields, used

    def hirsch_finish(self, eshift):
        self._ck(self.lib.afq_hirsch_finish(self.h, float(numpy.real(eshift))))

    # ---- back-propagation
    def bp_configure(self, nbp):
        self._ck(self.lib.afq_bp_configure(self.h, int(nbp)))
        self.nbp = int(nbp)

    def bp_steps(self):
        out = numpy.zeros(self.nw, dtype=numpy.int32)
        self._ck(self.lib.afq_bp_steps(self.h, _p(out)))
        return out

    def local_energy_full_g(self, G):
        """(E, E1b, E2b) of Green's functions G[n, 2, M, M] by the full-G Cholesky energy."""
        G = _c128(G)
        n = G.shape[0]
        G = _c128(G, (n, 2, self.M, self.M))
        out = numpy.zeros((n, 3), dtype=numpy.complex128)
        self._ck(self.lib.afq_local_energy_full_g(self.h, _p(G), n, _p(out)))
        return out

    def ueg_pair_sums(self, G):
        """(E [n, 3], two_rdm [n, 2, 2, nq]) of general Green's functions G[n, 2, M, M] on a UEG handle: the pair sums
        of local_energy_ueg(system, G, two_rdm=...) per momentum transfer (afq_ueg_pair_sums; E without ecore)."""
        G = _c128(G)
        n = G.shape[0]
        G = _c128(G, (n, 2, self.M, self.M))
        E = numpy.zeros((n, 3), dtype=numpy.complex128)
        two = numpy.zeros((n, 2, 2, getattr(self, 'nq', 0)), dtype=numpy.complex128)
        self._ck(self.lib.afq_ueg_pair_sums(self.h, _p(G), n, _p(E), _p(two)))
        return E, two

    def hubbard_energy_full_g(self, G):
        """(E, E1b, E2b) of Green's functions G[n, 2, M, M] by local_energy_hubbard (afq_hubbard_energy_full_g)."""
        G = _c128(G)
        n = G.shape[0]
        G = _c128(G, (n, 2, self.M, self.M))
        out = numpy.zeros((n, 3), dtype=numpy.complex128)
        self._ck(self.lib.afq_hubbard_energy_full_g(self.h, _p(G), n, _p(out)))
        return out

    def correlations_full_g(self, G):
        """corr [n, 5, M, M] of general Green's functions G[n, 2, M, M] (afq_correlations_full_g): <n_is n_jt> in the
        slices 2s+t, <S+_i S-_j> in slice 4.  Any handle whose system is set."""
        G = _c128(G)
        n = G.shape[0]
        G = _c128(G, (n, 2, self.M, self.M))
        out = numpy.zeros((n, 5, self.M, self.M), dtype=numpy.complex128)
        self._ck(self.lib.afq_correlations_full_g(self.h, _p(G), n, _p(out)))
        return out

    def set_pairing_bonds(self, nbr):
        """afq_set_pairing_bonds: the bond table nbr int [nb, M] of the pairing correlations, nbr[b][i] = the partner
        site of i along bond b or -1 (estimators.pairing.lattice_bonds builds a lattice's); None or an empty table
        clears it.  A window in pairing mode leaves it: bp_observables(two_rdm='pairing') again afterwards."""
        if nbr is None or numpy.size(nbr) == 0:
            self._ck(self.lib.afq_set_pairing_bonds(self.h, 0, None))
            self._pair_nb = 0
            return
        if numpy.ndim(nbr) != 2 or numpy.shape(nbr)[1] != self.M:
            raise ValueError("pairing bonds: an integer array [nb, M]")
        nbr = numpy.ascontiguousarray(nbr, dtype=numpy.int32)
        self._ck(self.lib.afq_set_pairing_bonds(self.h, nbr.shape[0], _p(nbr)))
        self._pair_nb = nbr.shape[0]

    def pairing_full_g(self, G):
        """pair [n, nb, nb, M, M] of general Green's functions G[n, 2, M, M] (afq_pairing_full_g) over the table of
        set_pairing_bonds: pair[b, b', i, j] = G_0[i, j] G_1[nbr[b][i], nbr[b'][j]] = <D+(i, i_b) D(j, j_b')> with
        D+(k, l) = c+_k,up c+_l,down for G[i,j] = <c+_i c_j>, 0 where a partner is -1; for the transposed convention
        the element [b, b', i, j] is pair[b', b, j, i].  Any handle with a system and a bond table."""
        G = _c128(G)
        n = G.shape[0]
        G = _c128(G, (n, 2, self.M, self.M))
        nb = getattr(self, '_pair_nb', 0)
        out = numpy.zeros((n, nb, nb, self.M, self.M), dtype=numpy.complex128)
        self._ck(self.lib.afq_pairing_full_g(self.h, _p(G), n, _p(out)))
        return out

    def bp_observables(self, two_rdm=False, ekt=False, h1=None, L=None):
        """afq_bp_observables: what bp_update may be asked for.  EKT: h1 [M, M] and L [nL, M, M] (None: a generic
        system's own vectors).  two_rdm='structure_factor' (UEG): bp_update's 'two_rdm' then is [2, 2, nq];
        two_rdm='correlation' (any system): [5, M, M], the weighted sum of correlations_full_g over the walkers;
        two_rdm='pairing' (any system, after set_pairing_bonds; afq_bp_pairing): [nb, nb, M, M], the weighted sum of
        pairing_full_g over the walkers."""
        if isinstance(two_rdm, str) and two_rdm not in ('structure_factor', 'correlation', 'pairing'):
            raise ValueError("two_rdm: True, 'structure_factor', 'correlation' or 'pairing'")
        self._bp_sf = isinstance(two_rdm, str) and two_rdm == 'structure_factor'
        self._bp_corr = isinstance(two_rdm, str) and two_rdm == 'correlation'
        self._bp_pair = isinstance(two_rdm, str) and two_rdm == 'pairing'
        two_rdm = 2 if self._bp_sf else 3 if self._bp_corr else 0 if self._bp_pair else int(bool(two_rdm))
        M = self.M
        h1p = Lp = None
        nL = 0
        if ekt:
            h1 = _c128(h1, (M, M))
            h1p = _p(h1)
            if L is None:
                nL = self.K
            else:
                L = _c128(L)
                nL = L.shape[0]
                L = _c128(L, (nL, M, M))
                Lp = _p(L)
        self._ck(self.lib.afq_bp_observables(self.h, two_rdm, int(bool(ekt)), h1p, Lp, int(nL)))
        if self._bp_pair:
            self._ck(self.lib.afq_bp_pairing(self.h, 1))

    def bp_ekt_chunks(self, nc=0, ncy=0):
        """afq_bp_ekt_chunks: Cholesky vectors per EKT chunk (0: automatic)."""
        self._ck(self.lib.afq_bp_ekt_chunks(self.h, int(nc), int(ncy)))

    def bp_update(self, phi_bp0, nstblz, restore_weights=None, eval_energy=False, reset=True, two_rdm=False,
                  ekt=False):
        """-> (energies_sum[3], denominator, G_bp_sum[2, M, M]); restore_weights in (None, 'partial', 'full').
        With two_rdm / ekt (after bp_observables) a fourth item {'two_rdm': [M]*4, 'fock_1p': [M, M], 'fock_1h':
        [M, M]} holds the weighted sums of what was asked for ('two_rdm': [2, 2, nq] after
        bp_observables(two_rdm='structure_factor'), [5, M, M] after bp_observables(two_rdm='correlation'),
        [nb, nb, M, M] after bp_observables(two_rdm='pairing'))."""
        mode = {None: 0, 'partial': 1, 'full': 2}.get(restore_weights, 1)
        phi0 = _c128(phi_bp0, (self.M, self.na + self.nb))
        M = self.M
        out = numpy.zeros(4 + 2 * M * M, dtype=numpy.complex128)
        if not (two_rdm or ekt):
            self._ck(self.lib.afq_bp_update(self.h, _p(phi0), int(nstblz), mode, int(bool(eval_energy)),
                                            int(bool(reset)), _p(out)))
            return out[:3], out[3], out[4:].reshape(2, M, M)
        two = None
        if two_rdm:
            shape = ((2, 2, self.nq) if getattr(self, '_bp_sf', False)
                     else (5, M, M) if getattr(self, '_bp_corr', False)
                     else (self._pair_nb, self._pair_nb, M, M) if getattr(self, '_bp_pair', False) else (M, M, M, M))
            two = numpy.zeros(shape, dtype=numpy.complex128)
        fock = numpy.zeros((2, M, M), dtype=numpy.complex128) if ekt else None
        self._ck(self.lib.afq_bp_update_ext(self.h, _p(phi0), int(nstblz), mode, int(bool(eval_energy)),
                                            int(bool(reset)), _p(out), None if two is None else _p(two),
                                            None if fock is None else _p(fock)))
        extra = {'two_rdm': two}
        if fock is not None:
            extra['fock_1p'], extra['fock_1h'] = fock[0], fock[1]
        return out[:3], out[3], out[4:].reshape(2, M, M), extra

    def bp_update_msd(self, dets, coeffs, nstblz, restore_weights=None, eval_energy=False, reset=True):
        """The window of a multi-determinant trial (afq_bp_update_msd): dets [ndet, M, na+nb], coeffs [ndet] ->
        (energies_sum[3], denominator, G_bp_sum[2, M, M], detw[nw, ndet]) with detw = w_d / sum_d w_d per walker."""
        mode = {None: 0, 'partial': 1, 'full': 2}.get(restore_weights, 1)
        dets = _c128(dets)
        ndet = dets.shape[0]
        dets = _c128(dets, (ndet, self.M, self.na + self.nb))
        coeffs = _c128(coeffs, (ndet,))
        M = self.M
        out = numpy.zeros(4 + 2 * M * M, dtype=numpy.complex128)
        detw = numpy.zeros((self.nw, ndet), dtype=numpy.complex128)
        self._ck(self.lib.afq_bp_update_msd(self.h, int(ndet), _p(dets), _p(coeffs), int(nstblz), mode,
                                            int(bool(eval_energy)), int(bool(reset)), _p(out), _p(detw)))
        return out[:3], out[3], out[4:].reshape(2, M, M), detw

    # ---- imaginary-time Green's function
    def itcf_configure(self, nmax, neqlb=0, stable=True, restore_weights=False):
        """afq_itcf_configure: windows of nmax + neqlb steps on the field history (sized here when none is set)."""
        self._ck(self.lib.afq_itcf_configure(self.h, int(nmax), int(neqlb), int(bool(stable)), int(bool(restore_weights))))
        self.nbp = int(nmax) + int(neqlb)
        self.itcf_nmax = int(nmax)

    def itcf_update(self, psi_T, nstblz):
        """One window -> (spgf_sum [nmax+1, 2, 2, M, M], denominator): sum_w wfac_w Re G_w(tau) and sum_w wfac_w."""
        psi = _c128(psi_T, (self.M, self.na + self.nb))
        M = self.M
        # (before itcf_configure the library refuses with AFQ_ESTATE and writes nothing)
        spgf = numpy.zeros((getattr(self, 'itcf_nmax', 0) + 1, 2, 2, M, M), dtype=numpy.complex128)
        den = numpy.zeros(1, dtype=numpy.complex128)
        self._ck(self.lib.afq_itcf_update(self.h, _p(psi), int(nstblz), _p(spgf), _p(den)))
        return spgf, den[0]

    def set_trial_multi(self, psi, coeffs, rchol):
        """psi [ndet, M, na+nb], coeffs [ndet], rchol [ndet * (na+nb) M, K] (stacked per determinant)."""
        nt = self.na + self.nb
        psi = _c128(psi)
        ndet = psi.shape[0]
        psi = _c128(psi, (ndet, self.M, nt))
        coeffs = _c128(coeffs, (ndet,))
        rchol = _c128(rchol, (ndet * nt * self.M, self.K))
        self._ck(self.lib.afq_set_trial_multi(self.h, ndet, _p(psi), _p(coeffs), _p(rchol)))
        self.ndet = ndet

    def det_weights(self):
        """conj(c_d) <D_d|phi_w> of the last Green's function / overlap evaluation, [nw, ndet]."""
        out = numpy.zeros((self.nw, self.ndet), dtype=numpy.complex128)
        self._ck(self.lib.afq_walkers_det_weights(self.h, _p(out)))
        return out

    def set_propagator(self, BH1, mf_shift, dt, exp_order=6, hybrid=True, force_bias=True,
                       free_projection=False, hubbard_spin=False):
        BH1 = _c128(BH1, (2, self.M, self.M))
        mf = _c128(mf_shift, (self.K,))
        flags = ((L.AFQ_PROP_HYBRID if hybrid else 0) | (L.AFQ_PROP_FORCE_BIAS if force_bias else 0) |
                 (L.AFQ_PROP_FREE_PROJECTION if free_projection else 0) |
                 (L.AFQ_PROP_HUBBARD_SPIN if hubbard_spin else 0))
        self._ck(self.lib.afq_set_propagator(self.h, _p(BH1), _p(mf), float(dt), int(exp_order), flags))
        nv = ctypes.c_int()
        self._ck(self.lib.afq_vhs_count(self.h, ctypes.byref(nv)))
        self.nv = nv.value

    # -- walkers ----------------------------------------------------------
    def walkers_alloc(self, nw):
        self._ck(self.lib.afq_walkers_alloc(self.h, int(nw)))
        self.nw = int(nw)

    def _field_spec(self, field):
        M, nt, K = self.M, self.na + self.nb, self.K
        return {
            L.F_PHI: ((M, nt), numpy.complex128), L.F_WEIGHT: ((), numpy.float64),
            L.F_UNSCALED_WEIGHT: ((), numpy.float64), L.F_OT: ((), numpy.complex128),
            L.F_HYBRID_ENERGY: ((), numpy.complex128), L.F_PHASE: ((), numpy.complex128),
            L.F_DETR: ((), numpy.float64), L.F_ELOC: ((), numpy.complex128),
            L.F_GHALF: ((nt, M), numpy.complex128), L.F_G: ((2, M, M), numpy.complex128),
            L.F_XBAR: ((K,), numpy.complex128), L.F_XSHIFTED: ((K,), numpy.complex128),
            L.F_ENERGY: ((3,), numpy.complex128), L.F_LOG_DETR: ((), numpy.float64),
            L.F_THERMAL_G: ((2, M, M), getattr(self, 'thermal_dtype', numpy.float64)),
            L.F_THERMAL_STACK: ((getattr(self, 'thermal_nbins', 0), 2, M, M), getattr(self, 'thermal_dtype', numpy.float64)),
            L.F_THERMAL_RIGHT: ((2, M, M), numpy.complex128),
            L.F_THERMAL_M0: ((2,), numpy.complex128),
            L.F_THERMAL_DET: ((2,), numpy.complex128),
            L.F_CMF: ((), numpy.complex128), L.F_CFB: ((), numpy.complex128),
        }[field]

    def set(self, field, values, first=0):
        shape, dt = self._field_spec(field)
        values = numpy.ascontiguousarray(values, dtype=dt)
        if values.shape == shape:
            values = values.reshape((1,) + shape)
        assert values.shape[1:] == shape, (values.shape, shape)
        self._ck(self.lib.afq_walkers_set(self.h, field, _p(values), int(first), values.shape[0]))

    def get(self, field, first=0, count=None):
        shape, dt = self._field_spec(field)
        count = self.nw - first if count is None else count
        out = numpy.empty((count,) + shape, dtype=dt)
        self._ck(self.lib.afq_walkers_get(self.h, field, _p(out), int(first), int(count)))
        return out

    # -- thermal walkers (finite temperature) ------------------------------
    def thermal_configure(self, ntime_slices, stack_size, nstblz, BT, BT_inv, BH1, auxf, options=0):
        M = self.M
        BT, BT_inv, BH1 = _f64(BT, (2, M, M)), _f64(BT_inv, (2, M, M)), _f64(BH1, (2, M, M))
        auxf = _f64(auxf, (2, 2))
        self._ck(self.lib.afq_thermal_configure(self.h, int(ntime_slices), int(stack_size), int(nstblz), _p(BT),
                                                _p(BT_inv), _p(BH1), _p(auxf), int(options)))
        self.thermal_nbins = int(ntime_slices) // int(stack_size)
        self.thermal_dtype = numpy.float64

    def thermal_configure_continuous(self, ntime_slices, stack_size, dt, BT, BT_inv, BH1, mf_shift, fb_bound=1.0,
                                     options=0):
        """UEG with continuous fields: the walkers' G and bins are complex from here on."""
        M = self.M
        BT, BT_inv, BH1 = _f64(BT, (2, M, M)), _f64(BT_inv, (2, M, M)), _f64(BH1, (2, M, M))
        mf_shift = _c128(mf_shift, (self.K,))
        self._ck(self.lib.afq_thermal_configure_continuous(self.h, int(ntime_slices), int(stack_size), float(dt), _p(BT),
                                                           _p(BT_inv), _p(BH1), _p(mf_shift), float(fb_bound),
                                                           int(options)))
        self.thermal_nbins = int(ntime_slices) // int(stack_size)
        self.thermal_dtype = numpy.complex128

    def thermal_configure_hubbard_continuous(self, ntime_slices, stack_size, dt, BT, BT_inv, BH1, mf_shift, mf_const_fac,
                                             options=0):
        """Hubbard with continuous fields (dense trial, dense BH1): the walkers' G and bins are complex from here on."""
        M = self.M
        BT, BT_inv, BH1 = _f64(BT, (2, M, M)), _f64(BT_inv, (2, M, M)), _f64(BH1, (2, M, M))
        mf_shift = _c128(mf_shift, (M,))
        mfc = _c128(numpy.array([mf_const_fac]), (1,))
        self._ck(self.lib.afq_thermal_configure_hubbard_continuous(self.h, int(ntime_slices), int(stack_size), float(dt),
                                                                   _p(BT), _p(BT_inv), _p(BH1), _p(mf_shift), _p(mfc),
                                                                   int(options)))
        self.thermal_nbins = int(ntime_slices) // int(stack_size)
        self.thermal_dtype = numpy.complex128

    def thermal_propagate_continuous(self, xi=None, fetch_fields=False):
        """One slice of every walker; xi [nw, K] or None for the device's stream.  -> the fields used, when asked for."""
        if xi is not None:
            xi = _f64(xi, (self.nw, self.K))
        out = numpy.empty((self.nw, self.K), dtype=numpy.float64) if fetch_fields else None
        self._ck(self.lib.afq_thermal_propagate_continuous(self.h, _p(xi), _p(out)))
        return out

    def thermal_reset(self):
        self._ck(self.lib.afq_thermal_reset(self.h))

    def thermal_propagate(self, u, eshift=0.0, fetch_fields=False):
        u = _f64(u, (self.nw, self.M))
        fields = numpy.empty((self.nw, self.M), dtype=numpy.int32) if fetch_fields else None
        self._ck(self.lib.afq_thermal_propagate(self.h, _p(u), _p(fields), float(eshift)))
        return fields

    def thermal_greens(self, slice_ix):
        self._ck(self.lib.afq_thermal_greens(self.h, int(slice_ix)))

    def thermal_energy(self):
        """(E [nw, 3] = (E, T, V), nav [nw]) of the walkers' current G."""
        E = numpy.empty((self.nw, 3), dtype=numpy.float64)
        nav = numpy.empty(self.nw, dtype=numpy.float64)
        self._ck(self.lib.afq_thermal_energy(self.h, _p(E), _p(nav)))
        return E, nav

    def thermal_estimates(self, average_gf=False, one_rdm=False, two_rdm=False, per_bin=False):
        """The mixed estimator's sums of the thermal population (afq_thermal_estimates) -> dict:
        'cols' [nw, 4] = (E, T, V, nav) per walker -- with average_gf their sums over the Green's functions at
        slice_ix = ts * stack_size, ts = 0 .. nbins - 1, in that order; 'per_bin' [nbins, nw, 4] (one row without
        average_gf) when asked for; 'one_rdm' [2, M, M] = sum_w weight_w Re G_w and 'two_rdm' [2, 2, nq] (UEG) =
        sum_w weight_w Re two_rdm[P_w] of the G the call leaves: the last of the sweep, or the one at the current slice."""
        what = ((L.THERMAL_EST_AVERAGE_GF if average_gf else 0) | (L.THERMAL_EST_ONE_RDM if one_rdm else 0)
                | (L.THERMAL_EST_TWO_RDM if two_rdm else 0))
        nb = getattr(self, 'thermal_nbins', 1) if average_gf else 1
        out = {'cols': numpy.zeros((self.nw, 4), dtype=numpy.float64)}
        if per_bin:
            out['per_bin'] = numpy.zeros((nb, self.nw, 4), dtype=numpy.float64)
        if one_rdm:
            out['one_rdm'] = numpy.zeros((2, self.M, self.M), dtype=numpy.float64)
        if two_rdm:
            out['two_rdm'] = numpy.zeros((2, 2, getattr(self, 'nq', 0)), dtype=numpy.float64)
        self._ck(self.lib.afq_thermal_estimates(self.h, what, _p(out['cols']), _p(out.get('per_bin')),
                                                _p(out.get('one_rdm')), _p(out.get('two_rdm'))))
        return out

    def thermal_device_allocations(self):
        """Device blocks the handle has allocated so far (afq_thermal_device_allocations)."""
        out = numpy.zeros(1, dtype=numpy.int64)
        self._ck(self.lib.afq_thermal_device_allocations(self.h, _p(out)))
        return int(out[0])

    def thermal_set_sweep_budget(self, nbytes=0):
        """Bytes of scratch (G, P and the streamed T) the averaged sweep takes at a time; 0: the library's default."""
        self._ck(self.lib.afq_thermal_set_sweep_budget(self.h, int(nbytes)))

    def thermal_state(self):
        """(time slice, block, in-bin counter, nbins)."""
        out = numpy.zeros(4, dtype=numpy.int32)
        self._ck(self.lib.afq_thermal_state(self.h, _p(out)))
        return tuple(int(x) for x in out)

    # -- hot path ---------------------------------------------------------
    def greens(self, want_G=False, fetch=True):
        out = numpy.empty(self.nw, dtype=numpy.complex128) if fetch else None
        self._ck(self.lib.afq_greens(self.h, int(bool(want_G)), _p(out)))
        return out

    def calc_overlap(self, fetch=True):
        out = numpy.empty(self.nw, dtype=numpy.complex128) if fetch else None
        self._ck(self.lib.afq_calc_overlap(self.h, _p(out)))
        return out

    def propagate(self, xi, eshift):
        if xi is not None:
            xi = _f64(xi, (self.nw, self.K))
        es = complex(eshift)
        self._ck(self.lib.afq_propagate(self.h, _p(xi), es.real, es.imag))

    def propagate_begin(self, xi):
        """Everything of a step that does not read the energy shift (afq_propagate_begin)."""
        if xi is not None:
            xi = _f64(xi, (self.nw, self.K))
        self._ck(self.lib.afq_propagate_begin(self.h, _p(xi)))

    def propagate_finish(self, eshift):
        es = complex(eshift)
        self._ck(self.lib.afq_propagate_finish(self.h, es.real, es.imag))

    def reortho(self, fetch=True):
        out = numpy.empty(self.nw, dtype=numpy.float64) if fetch else None
        self._ck(self.lib.afq_reortho(self.h, _p(out)))
        return out

    def set_log_shift(self, on, log_shift=0.0, detR_shift=0.0):
        """use_log_shift (walkers/handler.py:45): walker.log_shift / walker.detR_shift of every walker."""
        self._ck(self.lib.afq_set_log_shift(self.h, int(bool(on)), float(log_shift), float(detR_shift)))

    def log_ovlp_sums(self):
        """sums of |ot|, |detR|, |log_detR| over this rank's walkers (walkers/handler.py:457-462)."""
        out = numpy.empty(3, dtype=numpy.float64)
        self._ck(self.lib.afq_log_ovlp_sums(self.h, _p(out)))
        return out

    def local_energy(self, fetch=True):
        out = numpy.empty((self.nw, 3), dtype=numpy.complex128) if fetch else None
        self._ck(self.lib.afq_local_energy(self.h, _p(out)))
        return out

    def force_bias(self):
        out = numpy.empty((self.nw, self.K), dtype=numpy.complex128)
        self._ck(self.lib.afq_force_bias(self.h, _p(out)))
        return out

    def shift_fields(self, xi, xbar):
        xi = _f64(xi, (self.nw, self.K))
        xbar = _c128(xbar, (self.nw, self.K))
        xs = numpy.empty((self.nw, self.K), dtype=numpy.complex128)
        cmf = numpy.empty(self.nw, dtype=numpy.complex128)
        cfb = numpy.empty(self.nw, dtype=numpy.complex128)
        self._ck(self.lib.afq_shift_fields(self.h, _p(xi), _p(xbar), _p(xs), _p(cmf), _p(cfb)))
        return xs, cmf, cfb

    def vhs(self, xs):
        xs = _c128(xs, (self.nw, self.K))
        out = numpy.empty((self.nw, self.nv, self.M, self.M), dtype=numpy.complex128)
        self._ck(self.lib.afq_vhs(self.h, _p(xs), _p(out)))
        return out

    def apply_exponential(self, vhs):
        vhs = _c128(vhs, (self.nw, self.nv, self.M, self.M))
        self._ck(self.lib.afq_apply_exponential(self.h, _p(vhs)))

    def kinetic(self):
        self._ck(self.lib.afq_kinetic(self.h))

    # -- driver glue ------------------------------------------------------
    def cap_weights(self, frac, total_weight):
        self._ck(self.lib.afq_cap_weights(self.h, float(frac), float(total_weight)))

    def set_weight_cap(self, frac, total_weight=-1.0):
        """Cap applied by propagate() itself from now on (frac <= 0: off); see afq_set_weight_cap."""
        self._ck(self.lib.afq_set_weight_cap(self.h, float(frac), float(total_weight)))

    def popcontrol_comb(self, r, target, fetch=True):
        """Single rank, or a collective over the ranks of comm_init (parent_ix is then the global comb)."""
        if not fetch:        # asynchronous: the total weight stays on the device (cap_weights(frac, -1))
            self._ck(self.lib.afq_popcontrol_comb(self.h, float(r), float(target), None, None))
            return None, None
        pix = numpy.zeros(self.nw * getattr(self, 'comm_size', 1), dtype=numpy.int32)
        tw = ctypes.c_double(0.0)
        self._ck(self.lib.afq_popcontrol_comb(self.h, float(r), float(target), _p(pix), ctypes.byref(tw)))
        return pix, tw.value

    def popcontrol_pair_branch(self, u, target, min_weight, max_weight, fetch=True):
        """Single-rank pair branching from the uniforms u (at least nw // 2) -> (mult, ndraws, total weight);
        ``fetch=False`` only enqueues the event and returns (None, None, None)."""
        u = numpy.ascontiguousarray(u, dtype=numpy.float64).reshape(-1)
        args = (self.h, _p(u) if u.size else None, int(u.size), float(target), float(min_weight), float(max_weight))
        if not fetch:        # asynchronous: the total weight stays on the device (cap_weights(frac, -1))
            self._ck(self.lib.afq_popcontrol_pair_branch(*args, None, None, None))
            return None, None, None
        mult = numpy.ones(self.nw, dtype=numpy.int32)
        nd, tw = ctypes.c_int32(0), ctypes.c_double(0.0)
        self._ck(self.lib.afq_popcontrol_pair_branch(*args, _p(mult), ctypes.byref(nd), ctypes.byref(tw)))
        return mult, nd.value, tw.value

    def scale_weights(self, scale):
        self._ck(self.lib.afq_walkers_scale_weights(self.h, float(scale)))

    def reset_weights(self):
        self._ck(self.lib.afq_walkers_reset_weights(self.h))

    def copy_walker(self, src, dst):
        self._ck(self.lib.afq_walkers_copy(self.h, int(src), int(dst)))

    def pack_bytes(self):
        n = ctypes.c_int64()
        self._ck(self.lib.afq_walker_pack_bytes(self.h, ctypes.byref(n)))
        return n.value

    def pack(self, iw, dev_ptr):
        self._ck(self.lib.afq_walker_pack(self.h, int(iw), ctypes.c_void_p(dev_ptr)))

    def unpack(self, iw, dev_ptr):
        self._ck(self.lib.afq_walker_unpack(self.h, int(iw), ctypes.c_void_p(dev_ptr)))

    def estimates_update(self, eval_energy):
        self._ck(self.lib.afq_estimates_update(self.h, int(bool(eval_energy))))

    def estimates_rdm(self, on=True):
        self._ck(self.lib.afq_estimates_rdm(self.h, int(bool(on))))

    def estimates_rdm_get(self, zero=False):
        out = numpy.empty((2, self.M, self.M), dtype=numpy.float64)
        self._ck(self.lib.afq_estimates_rdm_get(self.h, _p(out), int(bool(zero))))
        return out

    def estimates_sf(self, on=True):
        """Mixed structure factor: energy updates also add sum_w weight_w Re two_rdm[G_w] (afq_estimates_sf)."""
        self._ck(self.lib.afq_estimates_sf(self.h, int(bool(on))))

    def estimates_sf_get(self, zero=False):
        out = numpy.empty((2, 2, self.nq), dtype=numpy.float64)
        self._ck(self.lib.afq_estimates_sf_get(self.h, _p(out), int(bool(zero))))
        return out

    def estimates_get(self, zero=False):
        out = numpy.empty(10, dtype=numpy.complex128)
        self._ck(self.lib.afq_estimates_get(self.h, _p(out), int(bool(zero))))
        return out

    def estimates_fuse_next(self):
        """The next propagate / propagate_finish takes the step's estimator terms along (no estimates_update(False))."""
        self._ck(self.lib.afq_estimates_fuse_next(self.h))

    def estimates_update_publish(self, eval_energy, zero=False):
        """estimates_update + estimates_get_begin in one summation launch (the step that ends a block)."""
        self._ck(self.lib.afq_estimates_update_publish(self.h, int(bool(eval_energy)), int(bool(zero))))

    def estimates_get_begin(self, zero=False):
        """Enqueue the fetch; work enqueued afterwards keeps running while estimates_get_end waits for the sums."""
        self._ck(self.lib.afq_estimates_get_begin(self.h, int(bool(zero))))

    def estimates_get_end(self):
        out = numpy.empty(10, dtype=numpy.complex128)
        self._ck(self.lib.afq_estimates_get_end(self.h, _p(out)))
        return out

    # -- library-owned communicator -----------------------------------------
    def comm_available(self):
        """librccl loadable in this process (no collective, no GPU work)."""
        return bool(self.lib.afq_comm_available())

    def comm_unique_id(self):
        buf = ctypes.create_string_buffer(128)
        rc = self.lib.afq_comm_unique_id(buf)
        if rc != 0:
            raise L.AfqError(rc, "afq_comm_unique_id failed (librccl not loadable?)")
        return buf.raw

    def comm_init(self, unique_id, rank, nranks):
        self._ck(self.lib.afq_comm_init(self.h, ctypes.c_char_p(unique_id), int(rank), int(nranks)))
        self.comm_rank, self.comm_size = int(rank), int(nranks)

    def comm_init_ipc(self, rank, nranks, allgather):
        """Communicator over mapped peer windows, no RCCL.  ``allgather(send_bytes) -> bytes of every rank
        concatenated`` is the caller's all-gather (its MPI / torch.distributed communicator): the bootstrap of the
        window handles, called on the host whenever the library (re)makes its windows."""
        def thunk(send, recv, nbytes, _user):
            try:
                out = allgather(ctypes.string_at(send, nbytes))
                if len(out) != nbytes * nranks:
                    return 1
                ctypes.memmove(recv, out, len(out))
                return 0
            except Exception:                                   # noqa: BLE001  (must not unwind through C)
                return 1
        self._ipc_thunk = L.ALLGATHER_FN(thunk)                 # kept alive as long as the communicator
        self._ck(self.lib.afq_comm_init_ipc(self.h, int(rank), int(nranks), self._ipc_thunk, None))
        self.comm_rank, self.comm_size = int(rank), int(nranks)

    def comm_destroy(self):
        self._ck(self.lib.afq_comm_destroy(self.h))
        self.comm_rank, self.comm_size = 0, 1

    def comm_set_transport(self, window):
        self._ck(self.lib.afq_comm_set_transport(self.h, 1 if window else 0))

    def comm_set_capacity(self, cap):
        self._ck(self.lib.afq_comm_set_capacity(self.h, int(cap)))

    def comm_set_timeout(self, seconds):
        """Wait budget of the kernels that wait for a peer (default 300 s; AFQ_COMM_TIMEOUT_S)."""
        self._ck(self.lib.afq_comm_set_timeout(self.h, float(seconds)))

    def comm_probe(self):
        """Collective known-answer round (all-gather, one slot per peer, all-reduce); raises AfqError(AFQ_ECOMM)."""
        bad = numpy.zeros(3, dtype=numpy.int64)
        self._ck(self.lib.afq_comm_probe(self.h, _p(bad)))
        return bad

    def comm_stats(self):
        out = numpy.zeros(L.AFQ_COMM_NSTATS, dtype=numpy.int64)
        self._ck(self.lib.afq_comm_stats(self.h, _p(out)))
        st = dict(zip(['max_transfer', 'events', 'capacity', 'overflow', 'rank', 'size', 'walkers_sent', 'bytes_sent',
                       'window', 'error', 'kind', 'window_memory'], out.tolist()))
        st['transport'] = 'peer windows' if st['window'] else 'ncclSend/ncclRecv'
        st['kind'] = {0: 'in-process', 1: 'rccl', 2: 'ipc'}.get(st['kind'], st['kind'])
        return st

    def estimates_allreduce(self, buf=None):
        """Sum over the ranks of the communicator: the device accumulators in place (buf None) or a host array."""
        if buf is None:
            self._ck(self.lib.afq_estimates_allreduce(self.h, None, 0))
            return None
        a = numpy.ascontiguousarray(buf, dtype=numpy.complex128)
        self._ck(self.lib.afq_estimates_allreduce(self.h, _p(a), a.size))
        return a

    def rng_normal(self, n):
        out = numpy.empty(int(n), dtype=numpy.float64)
        self._ck(self.lib.afq_rng_normal(self.h, _p(out), int(n)))
        return out

    def philox4x32(self, ctr_key):
        ck = numpy.ascontiguousarray(ctr_key, dtype=numpy.uint32).reshape(-1, 6)
        out = numpy.zeros((ck.shape[0], 4), dtype=numpy.uint32)
        self._ck(self.lib.afq_rng_philox4x32(self.h, _p(ck), _p(out), ck.shape[0]))
        return out

    def debug(self, sync_every_launch=False, markers=False):
        self._ck(self.lib.afq_debug(self.h, int(bool(sync_every_launch)), int(bool(markers))))

    def last_launch(self):
        """(text, queued, retired): safe to call from a watchdog thread while another thread is blocked in a sync."""
        buf = ctypes.create_string_buffer(1024)
        q, r = ctypes.c_uint64(), ctypes.c_uint64()
        self.lib.afq_last_launch(self.h, buf, 1024, ctypes.byref(q), ctypes.byref(r))
        return buf.value.decode(errors='replace'), q.value, r.value

    def guard_check(self):
        """AFQ_DEBUG_GUARD: compare the bands of every live device block of the handle with their pattern; what differs goes
        to the process-wide log (guard_report)."""
        self._ck(self.lib.afq_debug_guard_check(self.h))

    def guard_report(self):
        """(number of band violations this process has logged, their text)."""
        buf = ctypes.create_string_buffer(16384)
        n = int(self.lib.afq_debug_guard_report(buf, 16384))
        return n, buf.value.decode(errors='replace')

    def rng_seed(self, seed, stream=0):
        self._ck(self.lib.afq_rng_seed(self.h, int(seed), int(stream)))

    def counters(self, reset=False, n=4):
        """[nfb_trig, nhe_trig, flagged overlap matrices, closed-deal propagator walker steps] and with n = 8 also
        [.., one-spin exchange-energy walker evaluations, one-spin Green's functions, NaN determinant overlaps taken as zero,
        closed-shell walker steps of the large-system GEMM chain] (afq_counters_ext); [8] and [9] (n = 10): walker steps of
        the early overlap and of the step hand-over."""
        out = numpy.zeros(max(4, n), dtype=numpy.int64)
        self._ck(self.lib.afq_counters_ext(self.h, _p(out), int(max(4, n)), int(reset)))
        return out

    def enable_timers(self, on=True):
        self._ck(self.lib.afq_enable_timers(self.h, int(on)))

    def timers(self, reset=False):
        out = numpy.zeros(8, dtype=numpy.float64)
        self._ck(self.lib.afq_timers(self.h, _p(out), int(reset)))
        return dict(zip(['greens', 'one_body', 'force_bias', 'vhs', 'exponential', 'overlap_weight',
                         'reortho', 'energy'], out))

    def kernel_trace(self, on=True, kinds=None):
        """Event pairs around the hot kernels' launches: every kind, or only ``kinds`` (list of K_* constants)."""
        arg = int(bool(on))
        if on and kinds is not None:
            arg = sum(2 << int(k) for k in kinds)
        self._ck(self.lib.afq_kernel_trace(self.h, arg))

    def kernel_trace_stride(self, kind, stride):
        """Time only every ``stride``-th launch of ``kind`` (an event pair costs a few microseconds of pipeline bubble)."""
        self._ck(self.lib.afq_kernel_trace_stride(self.h, int(kind), int(stride)))

    def kernel_trace_get(self, kind, max_n=4096):
        """Durations [ms] of the traced launches of kernel ``kind`` (_lib.K_*)."""
        out = numpy.zeros(max_n, dtype=numpy.float64)
        n = ctypes.c_int()
        self._ck(self.lib.afq_kernel_trace_get(self.h, int(kind), _p(out), max_n, ctypes.byref(n)))
        return out[:min(n.value, max_n)]

    def launch_trace(self, on=True):
        """Event pairs around every launch, keyed by name (afq_launch_trace): a profile pass."""
        self._ck(self.lib.afq_launch_trace(self.h, int(bool(on))))

    def launch_trace_get(self):
        """{name: (launches, total ms)} of the launches recorded since launch_trace(True)."""
        cap = 256
        names = ctypes.create_string_buffer(cap * 96)
        ms = numpy.zeros(cap, dtype=numpy.float64)
        cnt = numpy.zeros(cap, dtype=numpy.int64)
        n = ctypes.c_int()
        self._ck(self.lib.afq_launch_trace_get(self.h, ctypes.cast(names, ctypes.c_void_p), len(names), _p(ms), _p(cnt),
                                               cap, ctypes.byref(n)))
        out, at = {}, 0
        for k in range(min(n.value, cap)):
            end = names.raw.index(b'\0', at)
            out[names.raw[at:end].decode()] = (int(cnt[k]), float(ms[k]))
            at = end + 1
        return out

    def kernel_issued_flops(self, kind):
        """Matrix-pipe flops of the last launch of ``kind`` (padding included, 3M products counted as 3)."""
        out = ctypes.c_double(0.0)
        self._ck(self.lib.afq_kernel_issued_flops(self.h, int(kind), ctypes.byref(out)))
        return float(out.value)

    def propagator_issued_flops(self):
        """(open, closed): matrix-pipe flops ONE walker issues in the fused propagator's open-shell / closed-shell deal."""
        a, b = ctypes.c_double(0.0), ctypes.c_double(0.0)
        self._ck(self.lib.afq_propagator_issued_flops(self.h, ctypes.byref(a), ctypes.byref(b)))
        return float(a.value), float(b.value)

    def set_exchange_algorithm(self, mode):
        """0 automatic, 1 T-intermediate (exx_kernel), 2 quadratic form (see afq_set_exchange_algorithm)."""
        self._ck(self.lib.afq_set_exchange_algorithm(self.h, int(mode)))

    def exchange_algorithm(self):
        m = ctypes.c_int()
        self._ck(self.lib.afq_exchange_algorithm(self.h, ctypes.byref(m)))
        return m.value

    def set_propagator_closed_form(self, mode):
        """0 automatic, 1 streamed closed-shell deal, 2 V resident in registers where eligible (see
        afq_set_propagator_closed_form)."""
        self._ck(self.lib.afq_set_propagator_closed_form(self.h, int(mode)))

    def set_step_fusion(self, mode):
        """An announced step's closing Green's function as the tail of the propagator's launch: 0 never, 1 behind the
        4-multiplication body (the bits of 0), 2 behind the 3-multiplication resident body (default; see afq_set_step_fusion)."""
        self._ck(self.lib.afq_set_step_fusion(self.h, int(mode)))

    def set_step_fusion_scope(self, scope):
        """Which steps of the shape class run that tail: 0 announced propagate() calls only (default), 1 every propagate()
        and propagate_begin() (see afq_set_step_fusion_scope)."""
        self._ck(self.lib.afq_set_step_fusion_scope(self.h, int(scope)))

    def set_step_tail_overlap(self, on):
        """Mode 2's tail takes the overlap matrix and its inverse from the resident body's closing pass (default on; off:
        the launch of before, bit for bit; counters(n=9)[8] counts the walker steps; see afq_set_step_tail_overlap)."""
        self._ck(self.lib.afq_set_step_tail_overlap(self.h, int(on)))

    def set_step_handover(self, on):
        """Mode 2's launch with the early overlap also makes the next step's opening one-body pass under its inversion, and
        a step that nothing has come between starts from it (default on; off: the launch of before; counters(n=10)[9] counts
        the walker steps; see afq_set_step_handover)."""
        self._ck(self.lib.afq_set_step_handover(self.h, int(on)))

    def propagator_closed_form(self):
        m = ctypes.c_int()
        self._ck(self.lib.afq_propagator_closed_form(self.h, ctypes.byref(m)))
        return m.value

    def set_msd_force_bias(self, mode):
        """0 automatic, 1 one contraction per determinant, 2 determinant-averaged G (see afq_set_msd_force_bias)."""
        self._ck(self.lib.afq_set_msd_force_bias(self.h, int(mode)))

    def msd_force_bias(self):
        m = ctypes.c_int()
        self._ck(self.lib.afq_msd_force_bias(self.h, ctypes.byref(m)))
        return m.value


# -- in-process communicator: several AfqDevice objects driven by one host thread -----------------------------
def _handle_array(devs):
    return (ctypes.c_void_p * len(devs))(*[d.h.value for d in devs])


def comm_init_local(devs):
    """devs[i] becomes rank i of one communicator (afq_comm_init_local)."""
    lib = devs[0].lib
    rc = lib.afq_comm_init_local(_handle_array(devs), len(devs))
    if rc != 0:
        raise L.AfqError(rc, lib.afq_last_error(devs[0].h).decode())
    for i, d in enumerate(devs):
        d.comm_rank, d.comm_size = i, len(devs)


def popcontrol_comb_local(devs, r, target, fetch=True):
    """walkers/handler.py:225-338 over the ranks of comm_init_local -> (global parent_ix, total weight)."""
    lib = devs[0].lib
    n = len(devs)
    if not fetch:
        rc = lib.afq_popcontrol_comb_local(_handle_array(devs), n, float(r), float(target), None, None)
        pix = tw = None
    else:
        pix = numpy.zeros(n * devs[0].nw, dtype=numpy.int32)
        tw = ctypes.c_double(0.0)
        rc = lib.afq_popcontrol_comb_local(_handle_array(devs), n, float(r), float(target), _p(pix), ctypes.byref(tw))
        tw = tw.value
    if rc != 0:
        raise L.AfqError(rc, lib.afq_last_error(devs[0].h).decode())
    return pix, tw


def estimates_allreduce_local(devs):
    lib = devs[0].lib
    rc = lib.afq_estimates_allreduce_local(_handle_array(devs), len(devs))
    if rc != 0:
        raise L.AfqError(rc, lib.afq_last_error(devs[0].h).decode())
