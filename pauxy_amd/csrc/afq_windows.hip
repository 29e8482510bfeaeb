// The window estimators of libafqmc_hip.so (see include/afqmc_hip.h): back-propagation and its observables
// (estimators/back_propagation.py), multi-determinant windows (k_bp_msd.hip), the imaginary-time Green's function
// (k_itcf.hip) and the energies of caller-supplied full Green's functions.  Host-side sequencing only.  The k_*
// launchers read their operands from the handle, so a window that has them work on something else lends the
// handle's fields for a scope (Lent, afq_internal.h): every exit of that scope puts the walk's own values back.
#include <algorithm>
#include <optional>
#include "afq_host.h"

namespace {

// Bump carver over a workspace counted in complex units.  take<T>(n) names the next n elements of T, rounded up to
// whole complex units (every part stays 16-byte aligned); over a null base the pass only sizes: off is the total.
struct Carver {
    cplx *base;
    size_t off = 0;
    template <class T = cplx> T *take(size_t n) {
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += (n * sizeof(T) + sizeof(cplx) - 1) / sizeof(cplx);
        return p;
    }
};

// ---- multi-determinant windows (k_bp_msd.hip)
struct BpMsdWs {
    cplx *dets, *coeffs, *ot, *ovlp, *detw, *S, *fac, *ghalf, *G, *gsum, *E, *esum, *stack;
    double *logr, *detR;
    size_t len;
};

// the window's scratch of an ndet-determinant handle: len complex units, the parts inside base (null: sizing only)
BpMsdWs bp_msd_carve(afq_handle *h, cplx *base) {
    const size_t n = h->nw, nd = h->ndet, per = (size_t)h->M * h->nt, g2 = (size_t)2 * h->M * h->M * n;
    Carver c{base};
    BpMsdWs w;
    w.dets = c.take(nd * per); w.coeffs = c.take(nd); w.ot = c.take(n); w.ovlp = c.take(nd * n); w.detw = c.take(n * nd);
    w.S = c.take(n); w.fac = c.take(2 * n); w.ghalf = c.take(n * per); w.G = c.take(g2); w.gsum = c.take(g2);
    w.E = c.take(3 * n); w.esum = c.take(3 * n);
    // the column-stacked products keep one more copy of the determinants (the fused propagator works in place)
    w.stack = c.take(k_prop_fused_supported(h) ? 0 : nd * n * per);
    w.logr = c.take<double>(nd * n); w.detR = c.take<double>(nd * n);
    w.len = c.off;
    return w;
}

// ---- imaginary-time Green's function windows (k_itcf.hip)
struct ItcfWs {
    cplx *psiL, *psiR, *psiR2, *psiLc, *BT2inv, *B, *Binv, *P, *Q, *Ggr, *Gls, *T, *ws, *xs, *wfac, *est, *detm, *ovlp, *ot;
    cplx *ghalf, *G;
    double *f, *detR; int *dete;
    size_t len;
};

// the scratch of a window that keeps nkeep slices of psi_L, as bp_msd_carve
ItcfWs itcf_carve(afq_handle *h, cplx *base, int nkeep) {
    const size_t nw = h->nw, M = h->M, per = M * h->nt, mm = M * M, g2 = 2 * mm * nw;
    const bool gen = !h->hirsch;
    Carver c{base};
    ItcfWs w;
    w.psiL = c.take(nkeep * nw * per); w.psiR = c.take(nw * per); w.psiR2 = c.take(nw * per); w.psiLc = c.take(nw * per);
    w.BT2inv = c.take(2 * mm); w.B = c.take(g2); w.Binv = c.take(g2); w.P = c.take(g2); w.Q = c.take(g2);
    w.Ggr = c.take(g2); w.Gls = c.take(g2); w.T = c.take(g2);
    w.ws = c.take(gen ? 2 * nw * mm + g2 : 0);                  // the generic Taylor workspace
    w.xs = gen ? c.take(nw * h->K) : nullptr;                   // the fields of a generic step,
    w.f = gen ? nullptr : c.take<double>(4 * nw * M);           // or the discrete diagonals in their place
    w.wfac = c.take(nw);
    w.est = c.take(1 + (size_t)(h->it_nmax + 1) * 4 * mm);      // [denom | spgf]
    w.detm = c.take(nw + 2); w.dete = c.take<int>(4 * (nw + 2));    // determinants: mantissas, exponents (as many units)
    w.ovlp = c.take(nw);
    w.ot = c.take(nw); w.detR = c.take<double>(2 * nw);         // parked by the re-orthogonalisation (a unit per walker)
    w.ghalf = c.take(nw * per); w.G = c.take(g2);               // the Ghalf and the G of the window's Green's functions
    w.len = c.off;
    return w;
}

// the window's device scratch, kept on the handle and grown on demand (a larger window frees the old buffer first)
int itcf_scratch(afq_handle *h, size_t n, cplx **out) {
    const int rc = dev_grow(h, LT_WALKERS, &h->it_ws, &h->it_ws_len, n, "imaginary-time window");
    *out = h->it_ws;
    return rc;
}

// ---- the pieces every window is made of
// every walker's phi_bp <- psi_T (staged in the second half of phi_bp, which is free until the conjugate is taken)
int window_begin(afq_handle *h, const double *psi_T) {
    const size_t per = (size_t)h->M * h->nt, n = h->nw;
    AFQ_HIP(h, hipMemcpyAsync(h->phi_bp + per * n, psi_T, sizeof(cplx) * per, hipMemcpyHostToDevice, h->stream));
    return k_bp_init(h, h->phi_bp + per * n);
}

// with reset, FieldConfig.reset + Walkers.copy_historic_wfn (walkers/stack.py:124-127, handler.py:200-203): the next
// window starts from the walkers now; the alive flags go back to the walkers' either way
int window_end(afq_handle *h, bool reset) {
    int rc;
    if (reset) {
        if ((rc = k_bp_reset(h, false))) return rc;
        AFQ_HIP(h, hipMemcpyAsync(h->phi_old, h->phi, sizeof(cplx) * h->M * h->nt * h->nw, hipMemcpyDeviceToDevice, h->stream));
    }
    return k_alive(h);
}

// utils/linalg.py:82-105 on both spins of a phi that is not the walkers': their overlaps and detR are parked in ot and
// detR [nw], and no weight is touched (free projection off)
int reortho_foreign(afq_handle *h, cplx *phi, cplx *ot, double *detR) {
    Lent<cplx *> l_phi(h->phi, phi), l_ot(h->ot, ot);
    Lent<double *> l_detR(h->detR, detR);
    Lent<int> l_flags(h->flags, h->flags & ~AFQ_PROP_FREE_PROJECTION);
    return k_reortho(h);
}

// gab(L, R)^T per walker: the Green's function of R with L[w] (Lc its conjugate) in the role of the trial; overlaps to
// ovlp, Ghalf and G to the given destinations.  window_owned says whose they are:
//   false  the handle's own ghalf / G (the caller has run ensure_G): the bumped version stays, for what the walk had
//          cached is overwritten, and the caller leaves nothing kept
//   true   buffers of the window.  The handle's Ghalf is the walk's cached Green's function, which the next step and the
//          next re-orthogonalisation reuse (and with it whatever was contracted from it: GreensCache::Foreign),
//          and the handle's G is walker state of the mixed one_rdm (accumulated by every
//          estimator update, carried by comb, copy and pack).  The caller puts back what was kept once the
//          whole window has succeeded (GreensCache::ReadOnly).
int greens_with_trial(afq_handle *h, cplx *R, cplx *L, cplx *Lc, cplx *ovlp, cplx *ghalf, cplx *G, bool window_owned) {
    Lent<cplx *> l_phi(h->phi, R), l_psi(h->psi, L), l_psic(h->psic, Lc), l_ghalf(h->ghalf, ghalf), l_G(h->G, G);
    Lent<long> l_stride(h->psi_stride, (long)h->M * h->nt);
    std::optional<GreensCache::Foreign> foreign;
    if (window_owned) foreign.emplace(h->gf);
    int rc;
    if ((rc = k_greens(h, ovlp))) return rc;
    return k_full_G(h);
}

// phi_bp[d, w] <- B(x_0)^H ... B(x_{n-1})^H phi_bp[d, w] over the recorded history, for the nd determinant slabs of
// phi_bp with ONE field set and ONE HS potential per walker and step; every slab is re-orthogonalised after the i-th
// step from the end when i != 0 and i % nstblz == 0 (propagation/generic.py:279-288, hubbard.py:661-671).  Fused
// propagator: the slabs one after the other over that V.  GEMM chain: the step's own kernels for one slab, the
// determinants of a walker as one column-stacked operand for more (k_bp_msd_onebody / k_bp_msd_taylor through stack
// [nd, nw, M, nt]).  ot [nw] and detR [nd, nw] park what the re-orthogonalisations write; with logr [nd, nw], log det R
// of every (d, w) is added to it.  With keep (nd == 1), phi_bp after the step of window slice t (= nbp - 1 - i) is
// copied to keep + t nw M nt for t < nkeep (the ITCF's psi_L(t)).
int bp_backward(afq_handle *h, int nd, int nstblz, cplx *stack, cplx *ot, double *detR, double *logr, cplx *keep, int nkeep) {
    const size_t n = h->nw, per = (size_t)h->M * h->nt, slab = n * per;
    // borrow the step machinery: phi <- phi_bp, BH1 <- BH1^H, fields <- -conj(x), every walker "alive"
    // while it still has recorded steps; the walkers' own overlaps / detR / weights are parked
    Lent<cplx *> l_phi(h->phi, h->phi_bp), l_xs(h->xs, h->bp_xs), l_BH1(h->BH1, h->BH1dag), l_ot(h->ot, ot);
    Lent<double *> l_detR(h->detR, detR);
    Lent<int> l_flags(h->flags, h->flags & ~AFQ_PROP_FREE_PROJECTION);
    const bool fused = k_prop_fused_supported(h);
    cplx *A = h->phi_bp, *B = stack, *C = h->phi_bp + nd * slab;        // (the conjugates' half is free until the end)
    int rc;
    for (int i = 0; i < h->nbp; ++i) {                                  // propagation/generic.py:279-288
        if (h->hirsch) {                                                // propagation/hubbard.py:661-671
            if ((rc = k_bp_hirsch_step(h, i))) return rc;
        } else {
            if ((rc = k_bp_fields(h, i))) return rc;
            {
                Lent<bool> l_upper(h->step.vhs_upper, fused && h->hs_sym);
                if ((rc = build_vhs(h))) return rc;
                for (int d = 0; fused && d < nd; ++d) {
                    Lent<cplx *> l_slab(h->phi, A + d * slab);
                    if ((rc = k_prop_fused(h))) return rc;
                }
            }
            if (!fused && nd == 1) {
                if ((rc = k_onebody(h))) return rc;
                if ((rc = apply_exp(h, h->vhs))) return rc;
                if ((rc = k_onebody(h))) return rc;
            } else if (!fused) {
                if ((rc = k_bp_msd_onebody(h, nd, A, B))) return rc;
                if ((rc = k_bp_msd_taylor(h, nd, h->vhs, B, C, A))) return rc;
                if ((rc = k_bp_msd_onebody(h, nd, B, A))) return rc;
            }
        }
        if (i != 0 && i % nstblz == 0) {
            for (int d = 0; d < nd; ++d)
                if ((rc = reortho_foreign(h, A + d * slab, ot, detR + d * n))) return rc;
            if (logr && (rc = k_bp_msd_logr(h, detR, logr, (long)(nd * n)))) return rc;
        }
        const int t = h->nbp - 1 - i;
        if (keep && t < nkeep)
            AFQ_HIP(h, hipMemcpyAsync(keep + (size_t)t * slab, h->phi_bp, sizeof(cplx) * slab, hipMemcpyDeviceToDevice, h->stream));
    }
    return AFQ_OK;
}

// length of the two_rdm part of bpo_out in the mode afq_bp_observables set: the structure factor [2, 2, nq], the
// correlation functions [5, M, M] or the two-body RDM [M]^4; or, in the mode afq_bp_pairing set, the pairing correlations
// [nb, nb, M, M]
size_t bpo_two_len(const afq_handle *h) {
    const size_t m2 = (size_t)h->M * h->M;
    return h->bpo_sf ? (size_t)4 * h->nq : h->bpo_corr ? 5 * m2 : h->bpo_pair ? (size_t)h->pair_nb * h->pair_nb * m2 : m2 * m2;
}

int bp_update(afq_handle *h, const double *phi_bp0, int nstblz, int restore_weights, int eval_energy,
              int reset, double *est_out, double *two_rdm_out, double *fock_out) {
    drop_walk_caches(h);
    if (!h || !phi_bp0 || !est_out || nstblz < 1 || restore_weights < 0 || restore_weights > 2) return AFQ_EINVAL;
    int rc = need_ready(h, true);
    if (rc) return rc;
    if (!h->nbp) AFQ_FAIL(h, AFQ_ESTATE, "back-propagation is not configured");
    if (h->hirsch && restore_weights)
        AFQ_FAIL(h, AFQ_EUNSUPPORTED, "restore_weights with discrete fields: FieldConfig.push records no weight factors (walkers/stack.py:35-49)");
    const size_t per = (size_t)h->M * h->nt, n = h->nw;
    // trial (or initial) determinant for every walker
    if ((rc = window_begin(h, phi_bp0))) return rc;
    if ((rc = bp_backward(h, 1, nstblz, nullptr, h->bp_ot, h->bp_detR, nullptr, nullptr, 0))) return rc;
    // G_bp[w] = gab(phi_bp, phi_old)^T (back_propagation.py:156-157) = the Green's function of phi_old with
    // phi_bp[w] in the role of the trial, into the handle's own Ghalf and G
    cplx *conj_bp = h->phi_bp + per * n;
    if ((rc = k_conj_copy(h, h->phi_bp, conj_bp, (long)(per * n)))) return rc;
    if ((rc = ensure_G(h))) return rc;
    if ((rc = greens_with_trial(h, h->phi_old, h->phi_bp, conj_bp, h->ovlp_old, h->ghalf, h->G, false))) return rc;
    AFQ_HIP(h, hipMemsetAsync(h->bp_est, 0, sizeof(cplx) * ((size_t)4 + 2 * h->M * h->M), h->stream));
    if (eval_energy) {
        // local_energy(system, G_bp, opt=False) (back_propagation.py:159-163): the full-G Cholesky energy
        // Hubbard: estimators/hubbard.py:93-114 on G_bp; UEG: estimators/ueg.py:27-88 on G_bp (k_ueg_sf.hip), below
        if (h->kind == AFQ_SYS_GENERIC) { if ((rc = k_energy_full_g(h, h->G, h->nw, h->energy))) return rc; }
        else if (h->kind == AFQ_SYS_HUBBARD) { if ((rc = k_energy_hubbard_full_g(h, h->G, h->nw, h->energy))) return rc; }
    }
    const bool sf = two_rdm_out && h->bpo_sf;
    cplx *sf_two = nullptr, *sf_E = nullptr;
    if (h->kind == AFQ_SYS_UEG && (eval_energy || sf)) {
        // one evaluation serves both: the energies fold the per-q sums the structure factor keeps
        if ((rc = k_ueg_sf_two(h, h->nw, &sf_two, &sf_E))) return rc;
        if ((rc = k_ueg_pair_sums(h, h->G, h->nw, eval_energy ? h->energy : sf_E, sf_two))) return rc;
    }
    if ((rc = k_bp_accumulate(h, restore_weights, eval_energy))) return rc;
    const bool corr = two_rdm_out && h->bpo_corr, pair = two_rdm_out && h->bpo_pair;
    const size_t m2 = (size_t)h->M * h->M, m4 = bpo_two_len(h);
    if (two_rdm_out || fock_out) {
        // sum_w wt_w two_rdm[G_bp[w]] and (F1p, F1h)[G_bp[w]] (k_bp_obs.hip), before the reset clears the weight factors
        if ((rc = k_bp_observables(h, restore_weights, two_rdm_out && !sf && !corr && !pair ? h->bpo_out : nullptr,
                                   fock_out ? h->bpo_out + (h->bpo_two ? m4 : 0) : nullptr))) return rc;
        // the structure factor with the same weights (bpo_wt), walkers in index order
        if (sf && (rc = k_ueg_sf_wsum(h, sf_two, h->nw, h->bpo_wt, nullptr, h->bpo_out, nullptr))) return rc;
        // the correlation functions of every G_bp[w], summed with the same weights (k_corr.hip)
        if (corr && (rc = k_corr_wsum(h, h->G, h->nw, h->bpo_wt, h->bpo_out))) return rc;
        // the pairing correlations of every G_bp[w] over the handle's bond table, the same way (k_pair.hip)
        if (pair && (rc = k_pair_wsum(h, h->G, h->nw, h->bpo_wt, h->bpo_out))) return rc;
    }
    if ((rc = window_end(h, reset != 0))) return rc;
    if (two_rdm_out && (rc = copy_out(h, two_rdm_out, h->bpo_out, sizeof(cplx) * m4))) return rc;
    if (fock_out && (rc = copy_out(h, fock_out, h->bpo_out + (h->bpo_two ? m4 : 0), sizeof(cplx) * 2 * m2))) return rc;
    return copy_out(h, est_out, h->bp_est, sizeof(cplx) * ((size_t)4 + 2 * h->M * h->M));
}

// P = gab(psi_L, psi_R) per spin, Q = I - P: the Green's function of psi_R with psi_L[w] in the role of the trial, as the
// back-propagated G of bp_update, but into the window's own Ghalf and G
int itcf_greens(afq_handle *h, const ItcfWs &w, cplx *psiR, cplx *psiL) {
    int rc;
    if ((rc = k_conj_copy(h, psiL, w.psiLc, (long)h->M * h->nt * h->nw))) return rc;
    if ((rc = greens_with_trial(h, psiR, psiL, w.psiLc, w.ovlp, w.ghalf, w.G, true))) return rc;
    return k_itcf_projectors(h, w.G, w.P, w.Q);
}

// upload n full Green's functions [n, 2, M, M], run launch(G, E, T) on the device copies, copy out E [n, 3] and, with
// tsz, the launch's second result T [tsz]
template <class F> int full_g_call(afq_handle *h, const double *G, int n, double *E_out, size_t tsz, double *T_out, F launch) {
    hipSetDevice(h->device);
    DevTemp<cplx> Gd, Ed, Td;
    int rc = dev_temp(h, Gd, (size_t)2 * h->M * h->M * n, G);
    if (!rc) rc = dev_temp(h, Ed, (size_t)3 * n);
    if (!rc) rc = dev_temp(h, Td, tsz);
    if (!rc) rc = launch(Gd, Ed, Td);
    if (!rc) rc = copy_out(h, E_out, Ed, sizeof(cplx) * 3 * n);
    if (!rc && tsz) rc = copy_out(h, T_out, Td, sizeof(cplx) * tsz);
    return rc;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- back-propagation
int afq_bp_configure(afq_handle *h, int nbp) {
    if (!h || nbp < 1) return AFQ_EINVAL;
    if (th_thermal(h)) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: no back-propagation");
    int rc = need_ready(h, true);
    if (rc) return rc;
    if (h->ndet > 1 && h->kind != AFQ_SYS_GENERIC)
        AFQ_FAIL(h, AFQ_EUNSUPPORTED, "back-propagation of a multi-determinant trial: generic systems only");
    if (h->kind == AFQ_SYS_HUBBARD && !h->hirsch)
        AFQ_FAIL(h, AFQ_EUNSUPPORTED, "back-propagation of a Hubbard system: discrete fields only (the reference's propagation/hubbard.py:568-672 reads the history as 0 / 1 fields)");
    if (h->hirsch && h->K != h->M) AFQ_FAIL(h, AFQ_ESTATE, "discrete fields: one per site expected");
    if (h->flags & AFQ_PROP_FREE_PROJECTION) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "no field history in free projection");
    // the backward step reuses the forward one with fields -conj(x): B(x)^H only when every L_n^H == L_n
    if (h->hs_cplx == AFQ_HS_GENERAL)
        AFQ_FAIL(h, AFQ_EUNSUPPORTED, "back-propagation with non-Hermitian complex Cholesky vectors");
    const size_t per = (size_t)h->M * h->nt, n = h->nw, nd = h->ndet > 1 ? h->ndet : 1;
    size_t msd_ws = 0;
    if (nd > 1) {
        // the determinants' phi_bp (and conjugate) and the window's scratch are sized here, and checked first: a
        // configuration that does not fit says so with the byte counts instead of failing at an allocation half way
        msd_ws = bp_msd_carve(h, nullptr).len;
        size_t fr = 0, tot = 0;
        hipSetDevice(h->device);
        AFQ_HIP(h, hipMemGetInfo(&fr, &tot));
        const double need = 16.0 * ((double)2 * per * n * nd + (double)msd_ws + (double)n * nbp * h->K);
        if (need > 0.5 * (double)fr)
            AFQ_FAIL(h, AFQ_ENOMEM, "back-propagation of " + std::to_string(nd) + " determinants: " +
                                        std::to_string((unsigned long long)need) +
                                        " bytes, more than half of the free device memory (" +
                                        std::to_string((unsigned long long)fr) + " bytes)");
    }
    if ((rc = dev_alloc(h, LT_WALKERS, &h->bp_hist, n * nbp * h->K))) return rc;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->bp_n, n))) return rc;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->bp_flag, n))) return rc;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->bp_cos, n))) return rc;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->bp_ph, n))) return rc;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->phi_old, per * n))) return rc;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->phi_bp, 2 * per * n * nd))) return rc;   // phi_bp and conj(phi_bp), of every determinant
    if ((rc = dev_alloc(h, LT_WALKERS, &h->bp_ot, n))) return rc;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->bp_detR, n))) return rc;
    if (nd > 1) {
        if ((rc = dev_alloc(h, LT_WALKERS, &h->bpm_ws, msd_ws, "multi-determinant window", &h->bpm_ws_len))) return rc;
        h->bpm_ws_len = msd_ws;
    }
    if ((rc = dev_alloc(h, LT_WALKERS, &h->BH1dag, (size_t)2 * h->M * h->M))) return rc;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->bp_xs, n * h->K))) return rc;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->bp_est, (size_t)4 + 2 * h->M * h->M))) return rc;
    h->nbp = nbp;
    AFQ_HIP(h, hipMemsetAsync(h->bp_hist, 0, sizeof(cplx) * n * nbp * h->K, h->stream));
    AFQ_HIP(h, hipMemsetAsync(h->bp_flag, 0, sizeof(int) * n, h->stream));
    if ((rc = k_bp_reset(h, true))) return rc;
    if ((rc = k_conj_transpose(h, h->BH1, h->BH1dag))) return rc;
    // walkers/walker.py:43: phi_old starts as the walker itself
    AFQ_HIP(h, hipMemcpyAsync(h->phi_old, h->phi, sizeof(cplx) * per * n, hipMemcpyDeviceToDevice, h->stream));
    return AFQ_OK;
}

int afq_bp_steps(afq_handle *h, int32_t *steps_out) {
    if (!h || !steps_out) return AFQ_EINVAL;
    if (!h->nbp) AFQ_FAIL(h, AFQ_ESTATE, "back-propagation is not configured");
    hipSetDevice(h->device);
    int rc = copy_out(h, steps_out, h->bp_n, sizeof(int) * h->nw);
    // discrete fields are recorded one at a time: FieldConfig.step counts completed configurations
    if (!rc && h->hirsch) for (int i = 0; i < h->nw; ++i) steps_out[i] /= h->M;
    return rc;
}

int afq_bp_update(afq_handle *h, const double *phi_bp0, int nstblz, int restore_weights, int eval_energy,
                  int reset, double *est_out) {
    AFQ_API(h, "afq_bp_update");
    return bp_update(h, phi_bp0, nstblz, restore_weights, eval_energy, reset, est_out, nullptr, nullptr);
}

int afq_bp_update_ext(afq_handle *h, const double *phi_bp0, int nstblz, int restore_weights, int eval_energy,
                      int reset, double *est_out, double *two_rdm_out, double *fock_out) {
    AFQ_API(h, "afq_bp_update_ext");
    if (h && two_rdm_out && !h->bpo_two) AFQ_FAIL(h, AFQ_ESTATE, "two-body RDM: afq_bp_observables(h, 1, 2 or 3, ...) or afq_bp_pairing(h, 1) first");
    if (h && fock_out && !h->bpo_ekt) AFQ_FAIL(h, AFQ_ESTATE, "EKT Fock matrices: afq_bp_observables(h, ., 1, ...) first");
    return bp_update(h, phi_bp0, nstblz, restore_weights, eval_energy, reset, est_out, two_rdm_out, fock_out);
}

int afq_bp_update_msd(afq_handle *h, int ndet, const double *dets, const double *coeffs, int nstblz, int restore_weights,
                      int eval_energy, int reset, double *est_out, double *detw_out) {
    AFQ_API(h, "afq_bp_update_msd");
    // read-only on the walk, as afq_itcf_update: the Green's function the last step left for the next one stays valid
    GreensCache::ReadOnly read_only(h ? &h->gf : nullptr);
    if (h) h->step.handover.drop();     // (the window borrows phi and the step machinery)
    if (!h || !dets || !coeffs || !est_out || ndet < 1 || nstblz < 1 || restore_weights < 0 || restore_weights > 2)
        return AFQ_EINVAL;
    int rc = need_ready(h, true);
    if (rc) return rc;
    if (!h->nbp) AFQ_FAIL(h, AFQ_ESTATE, "back-propagation is not configured");
    if (h->ndet <= 1 || !h->bpm_ws)
        AFQ_FAIL(h, AFQ_ESTATE, "afq_bp_update_msd: the handle holds a single-determinant trial (afq_bp_update)");
    if (ndet != h->ndet)
        AFQ_FAIL(h, AFQ_EINVAL, "afq_bp_update_msd: " + std::to_string(ndet) + " determinants, the history was configured for " +
                                    std::to_string(h->ndet));
    const size_t per = (size_t)h->M * h->nt, n = h->nw, nd = ndet, slab = n * per, gsz = (size_t)2 * h->M * h->M;
    const BpMsdWs ws = bp_msd_carve(h, h->bpm_ws);
    AFQ_HIP(h, hipMemcpyAsync(ws.dets, dets, sizeof(cplx) * nd * per, hipMemcpyHostToDevice, h->stream));
    AFQ_HIP(h, hipMemcpyAsync(ws.coeffs, coeffs, sizeof(cplx) * nd, hipMemcpyHostToDevice, h->stream));
    AFQ_HIP(h, hipMemsetAsync(ws.logr, 0, sizeof(double) * nd * n, h->stream));
    for (size_t d = 0; d < nd; ++d) {   // every walker starts from D_d in slab d (k_bp_init fills the nw walkers phi_bp points at)
        Lent<cplx *> l_slab(h->phi_bp, h->phi_bp + d * slab);
        if ((rc = k_bp_init(h, ws.dets + d * per))) return rc;
    }
    if ((rc = bp_backward(h, ndet, nstblz, ws.stack, ws.ot, ws.detR, ws.logr, nullptr, 0))) return rc;
    // G_d[w] = gab(Q_d, phi_old)^T and <Q_d|phi_old> with Q_d[w] in the role of the trial, determinant by determinant
    // into the window's own Ghalf / G
    cplx *conj_bp = h->phi_bp + nd * slab;
    if ((rc = k_conj_copy(h, h->phi_bp, conj_bp, (long)(nd * slab)))) return rc;
    if (eval_energy && h->kind != AFQ_SYS_GENERIC) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "back-propagated energies: generic systems only");
    for (size_t d = 0; d < nd; ++d) {
        if ((rc = greens_with_trial(h, h->phi_old, h->phi_bp + d * slab, conj_bp + d * slab, ws.ovlp + d * n, ws.ghalf, ws.G, true)))
            return rc;
        if (eval_energy && (rc = k_energy_full_g(h, ws.G, h->nw, ws.E))) return rc;     // E[G_d], not E[G_bp]: quadratic in G
        if ((rc = k_bp_msd_detw(h, ndet, (int)d, ws.coeffs, ws.logr, ws.ovlp, ws.detw, ws.S))) return rc;
        if ((rc = k_bp_msd_gsum(h, ndet, (int)d, ws.detw, ws.G, ws.gsum, eval_energy ? ws.E : nullptr, ws.esum))) return rc;
    }
    AFQ_HIP(h, hipMemsetAsync(h->bp_est, 0, sizeof(cplx) * (4 + gsz), h->stream));
    if ((rc = k_bp_msd_finish(h, ndet, restore_weights, ws.detw, ws.S, ws.fac))) return rc;
    if ((rc = k_bp_msd_accumulate(h, ws.gsum, ws.fac, eval_energy ? ws.esum : nullptr, h->bp_est))) return rc;
    if ((rc = window_end(h, reset != 0))) return rc;
    read_only.succeeded();
    if ((rc = copy_out(h, detw_out, ws.detw, sizeof(cplx) * n * nd))) return rc;
    return copy_out(h, est_out, h->bp_est, sizeof(cplx) * (4 + gsz));
}

int afq_bp_ekt_chunks(afq_handle *h, int nc, int ncy) {
    if (!h || nc < 0 || ncy < 0) return AFQ_EINVAL;
    h->bpo_nc = nc; h->bpo_ncy = ncy;
    return AFQ_OK;
}

// share of the free device memory the M^4 two-body RDM (one copy on the device) may take
#define AFQ_BPO_MEM_SHARE 0.5

int afq_bp_observables(afq_handle *h, int two_rdm, int ekt, const double *h1, const double *L, int nL) {
    if (!h || (ekt && (!h1 || nL < 1 || (L == nullptr && nL != h->K)))) return AFQ_EINVAL;
    int rc = need_ready(h, true);
    if (rc) return rc;
    if (h->ndet > 1 && (two_rdm || ekt))
        AFQ_FAIL(h, AFQ_EUNSUPPORTED, "back-propagated two-body RDM / EKT with a multi-determinant trial (sum_d w_d f[G_d] of quartic / cubic forms)");
    if (!h->nbp) AFQ_FAIL(h, AFQ_ESTATE, "back-propagation is not configured: afq_bp_configure first");
    if (ekt && h->kind == AFQ_SYS_HUBBARD) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "EKT: the Hubbard model has no Cholesky vectors");
    if (two_rdm == 2 && h->kind != AFQ_SYS_UEG)
        AFQ_FAIL(h, AFQ_EUNSUPPORTED, "structure factor: UEG systems only (no momentum transfers elsewhere)");
    if (two_rdm < 0 || two_rdm > 3)
        AFQ_FAIL(h, AFQ_EINVAL, "afq_bp_observables: two_rdm is 0, 1 (two-body RDM), 2 (structure factor) or 3 (correlation functions)");
    const bool sf = two_rdm == 2, corr = two_rdm == 3;
    if (ekt && !L && h->kind != AFQ_SYS_GENERIC) AFQ_FAIL(h, AFQ_EINVAL, "EKT: pass the vectors L_x of this system");
    if (ekt && !L && h->hs_cplx)
        AFQ_FAIL(h, AFQ_EUNSUPPORTED, "EKT with complex Cholesky vectors: the reference's 4-fold-symmetry form pins nothing");
    const size_t M = (size_t)h->M, m4 = sf ? (size_t)4 * h->nq : corr ? 5 * M * M : M * M * M * M;
    hipSetDevice(h->device);
    dev_alloc(h, LT_WALKERS, &h->bpo_out, 0);      // a buffer of an earlier call does not count against the budget
    if (two_rdm && !sf && !corr) {
        size_t fr = 0, tot = 0;
        AFQ_HIP(h, hipMemGetInfo(&fr, &tot));
        const double need = 16.0 * (double)m4;
        if (need > AFQ_BPO_MEM_SHARE * (double)fr)
            AFQ_FAIL(h, AFQ_ENOMEM, "two-body RDM: " + std::to_string((unsigned long long)need) +
                                        " bytes (16 M^4) exceed half of the free device memory (" +
                                        std::to_string((unsigned long long)fr) + " bytes)");
    }
    dev_alloc(h, LT_WALKERS, &h->bpo_h1, 0); dev_alloc(h, LT_WALKERS, &h->bpo_L, 0);
    h->bpo_two = h->bpo_ekt = h->bpo_sf = h->bpo_corr = h->bpo_pair = 0; h->bpo_nL = 0;
    if (ekt) {
        if ((rc = dev_upload(h, LT_WALKERS, &h->bpo_h1, h1, M * M))) return rc;
        if (L && (rc = dev_upload(h, LT_WALKERS, &h->bpo_L, L, (size_t)nL * M * M))) return rc;
        h->bpo_nL = nL;
    }
    if ((two_rdm || ekt) && (rc = dev_alloc(h, LT_WALKERS, &h->bpo_out, (two_rdm ? m4 : 0) + (ekt ? 2 * M * M : 0)))) return rc;
    h->bpo_two = two_rdm ? 1 : 0; h->bpo_ekt = ekt ? 1 : 0; h->bpo_sf = sf ? 1 : 0; h->bpo_corr = corr ? 1 : 0;
    return AFQ_OK;
}

// ---------------------------------------------------------------- pairing correlations (k_pair.hip)
int afq_set_pairing_bonds(afq_handle *h, int nb, const int32_t *nbr) {
    if (!h || nb < 0 || (nb && !nbr)) return AFQ_EINVAL;
    if (!h->kind) AFQ_FAIL(h, AFQ_ESTATE, "pairing bonds: the system must be set (the table is [nb, M])");
    if (nb > 16) AFQ_FAIL(h, AFQ_EINVAL, "pairing bonds: " + std::to_string(nb) + " bonds, at most 16");
    const size_t M = (size_t)h->M;
    for (size_t e = 0; e < nb * M; ++e)
        if (nbr[e] < -1 || nbr[e] >= h->M)
            AFQ_FAIL(h, AFQ_EINVAL, "pairing bonds: nbr[" + std::to_string(e / M) + "][" + std::to_string(e % M) + "] = " +
                                        std::to_string(nbr[e]) + " is outside [-1, " + std::to_string(h->M) + ")");
    hipSetDevice(h->device);
    AFQ_HIP(h, hipStreamSynchronize(h->stream));   // queued work may still read the table that is replaced
    // a window in pairing mode was sized for the old table: the mode ends with it, the other modes stay
    if (h->bpo_pair) {
        h->bpo_pair = h->bpo_two = 0;
        int rc = dev_alloc(h, LT_WALKERS, &h->bpo_out, h->bpo_ekt ? 2 * M * M : 0);
        if (rc) return rc;
    }
    h->pair_nb = 0;
    int rc = dev_upload(h, LT_SYSTEM, &h->pair_nbr, nbr, nb * M);
    if (rc) return rc;
    h->pair_nb = nb;
    return AFQ_OK;
}

int afq_bp_pairing(afq_handle *h, int on) {
    if (!h) return AFQ_EINVAL;
    int rc = need_ready(h, true);
    if (rc) return rc;
    if (h->ndet > 1 && on)
        AFQ_FAIL(h, AFQ_EUNSUPPORTED, "back-propagated pairing correlations with a multi-determinant trial (sum_d w_d f[G_d] of a quadratic form)");
    if (!h->nbp) AFQ_FAIL(h, AFQ_ESTATE, "back-propagation is not configured: afq_bp_configure first");
    if (on && !h->pair_nb) AFQ_FAIL(h, AFQ_ESTATE, "pairing correlations: no bond table (afq_set_pairing_bonds first)");
    if (!on && !h->bpo_pair) return AFQ_OK;        // the two-body slot is in another mode or in none: left as it is
    // the two-body slot of the window changes its meaning; the EKT's operands and its slot behind it stay
    const size_t m2 = (size_t)h->M * h->M, m4 = on ? (size_t)h->pair_nb * h->pair_nb * m2 : 0;
    hipSetDevice(h->device);
    AFQ_HIP(h, hipStreamSynchronize(h->stream));
    h->bpo_two = h->bpo_sf = h->bpo_corr = h->bpo_pair = 0;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->bpo_out, m4 + (h->bpo_ekt ? 2 * m2 : 0), "pairing correlations"))) {
        h->bpo_ekt = 0;
        return rc;
    }
    h->bpo_two = h->bpo_pair = on ? 1 : 0;
    return AFQ_OK;
}

// ---------------------------------------------------------------- imaginary-time Green's function (k_itcf.hip)
int afq_itcf_configure(afq_handle *h, int nmax, int neqlb, int stable, int restore_weights) {
    if (!h || nmax < 1 || neqlb < 0) return AFQ_EINVAL;
    if (th_thermal(h)) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: no ITCF window");
    int rc = need_ready(h, true);
    if (rc) return rc;
    if (h->M > 128) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "ITCF: M > 128 (the batched Gauss-Jordan inverse)");
    if (h->kind == AFQ_SYS_UEG) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "ITCF: no propagator matrix for the UEG (itcf.py:114-122)");
    if (h->hirsch && restore_weights)
        AFQ_FAIL(h, AFQ_EUNSUPPORTED, "restore_weights with discrete fields: FieldConfig.push records no weight factors (walkers/stack.py:35-49)");
    if (h->ndet > 1) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "ITCF: multi-determinant trials");
    const int n = nmax + neqlb;
    if (h->nbp && h->nbp != n)
        AFQ_FAIL(h, AFQ_ESTATE, "ITCF: a field history of " + std::to_string(h->nbp) + " steps is configured, the window needs " +
                                    std::to_string(n));
    // (afq_bp_configure refuses continuous Hubbard fields, free projection and general complex Cholesky vectors)
    if (!h->nbp && (rc = afq_bp_configure(h, n))) return rc;
    h->it_nmax = nmax; h->it_neqlb = neqlb; h->it_stable = stable ? 1 : 0; h->it_restore = restore_weights ? 1 : 0;
    return AFQ_OK;
}

int afq_itcf_update(afq_handle *h, const double *psi_T, int nstblz, double *spgf_out, double *denom_out) {
    AFQ_API(h, "afq_itcf_update");
    // the window is read-only on the walk: the Green's function the last step left for the next one stays valid (a window
    // that fails half way leaves it invalid, which only costs a recomputation)
    GreensCache::ReadOnly read_only(h ? &h->gf : nullptr);
    if (h) h->step.handover.drop();     // (the window borrows phi and the step machinery)
    if (!h || !psi_T || !spgf_out || !denom_out || nstblz < 1) return AFQ_EINVAL;
    int rc = need_ready(h, true);
    if (rc) return rc;
    if (!h->it_nmax) AFQ_FAIL(h, AFQ_ESTATE, "ITCF is not configured: afq_itcf_configure first");
    if (h->nbp != h->it_nmax + h->it_neqlb) AFQ_FAIL(h, AFQ_ESTATE, "ITCF: the field history changed length");
    const int M = h->M, nw = h->nw, nmax = h->it_nmax;
    const size_t per = (size_t)M * h->nt, mm = (size_t)M * M, g2 = 2 * mm * nw, nspgf = (size_t)(nmax + 1) * 4 * mm;
    // psi_L(t) is read for every slice by the stable chain, for t = 0 only by the unstable one
    const bool stable = h->it_stable != 0;
    const int nkeep = stable ? nmax : 1;
    const bool gen = !h->hirsch;
    {
        size_t fr = 0, tot = 0;
        AFQ_HIP(h, hipMemGetInfo(&fr, &tot));
        const double need = 16.0 * (double)nw * nkeep * per;
        const double avail = (double)fr + 16.0 * (double)h->it_ws_len;   // (a buffer that has to grow is freed first)
        if (need > 0.5 * avail)
            AFQ_FAIL(h, AFQ_ENOMEM, "ITCF: the stored psi_L take " + std::to_string((unsigned long long)need) +
                                        " bytes, more than half of the free device memory (" +
                                        std::to_string((unsigned long long)avail) + " bytes)");
    }
    cplx *base;
    if ((rc = itcf_scratch(h, itcf_carve(h, nullptr, nkeep).len, &base))) return rc;
    const ItcfWs w = itcf_carve(h, base, nkeep);
    cplx *psiR = w.psiR, *psiR2 = w.psiR2, *Ggr = w.Ggr, *Gls = w.Gls, *T = w.T;     // (these trade places below)
    // BT2^-1 per spin
    AFQ_HIP(h, hipMemcpyAsync(w.BT2inv, h->BH1, sizeof(cplx) * 2 * mm, hipMemcpyDeviceToDevice, h->stream));
    if ((rc = k_gj_inverse(h, w.BT2inv, M, 2, w.detm, w.dete))) return rc;
    // 1. psi_L(t) = B_t^H psi_L(t+1) from psi_L(n) = psi_T: the back-propagation of bp_update, psi_L(t < nkeep) kept
    if ((rc = window_begin(h, psi_T))) return rc;
    if ((rc = bp_backward(h, 1, nstblz, nullptr, h->bp_ot, h->bp_detR, nullptr, w.psiL, nkeep))) return rc;
    // 2. weights of the window (the alive flags of the last backward step mark the walkers with a complete window)
    AFQ_HIP(h, hipMemsetAsync(w.est, 0, sizeof(cplx) * (1 + nspgf), h->stream));
    if ((rc = k_itcf_weights(h, h->it_restore, w.wfac, w.est))) return rc;
    // 3. forward: psi_R, P(t), the B matrices and the chains
    AFQ_HIP(h, hipMemcpyAsync(psiR, h->phi_old, sizeof(cplx) * nw * per, hipMemcpyDeviceToDevice, h->stream));
    for (int tau = 0; tau < nmax; ++tau) {
        if (stable || tau == 0) {
            if ((rc = itcf_greens(h, w, psiR, w.psiL + (size_t)tau * nw * per))) return rc;
        }
        if (tau == 0) {
            AFQ_HIP(h, hipMemcpyAsync(Ggr, w.Q, sizeof(cplx) * g2, hipMemcpyDeviceToDevice, h->stream));
            AFQ_HIP(h, hipMemcpyAsync(Gls, w.P, sizeof(cplx) * g2, hipMemcpyDeviceToDevice, h->stream));
            if ((rc = k_itcf_accumulate(h, Ggr, Gls, w.wfac, w.est + 1))) return rc;
        }
        if (gen) {
            {
                Lent<cplx *> l_xs(h->xs, w.xs);
                if ((rc = k_itcf_fields(h, w.xs, tau))) return rc;
                if ((rc = build_vhs(h))) return rc;
            }
            if ((rc = k_itcf_generic_b(h, h->vhs, h->BH1, w.BT2inv, w.B, w.Binv, w.ws, w.detm, w.dete))) return rc;
        } else {
            if ((rc = k_itcf_hirsch_b(h, tau, h->BH1, w.BT2inv, w.B, w.Binv, w.f))) return rc;
        }
        if (stable) {                                   // Ggr <- B (I - P) Ggr, Gls <- Gls P B^-1
            if ((rc = k_itcf_mul(h, w.Q, Ggr, T)) || (rc = k_itcf_mul(h, w.B, T, Ggr))) return rc;
            if ((rc = k_itcf_mul(h, Gls, w.P, T)) || (rc = k_itcf_mul(h, T, w.Binv, Gls))) return rc;
        } else {                                        // Ggr <- B Ggr, Gls <- Gls B^-1
            if ((rc = k_itcf_mul(h, w.B, Ggr, T))) return rc;
            std::swap(Ggr, T);
            if ((rc = k_itcf_mul(h, Gls, w.Binv, T))) return rc;
            std::swap(Gls, T);
        }
        if ((rc = k_itcf_accumulate(h, Ggr, Gls, w.wfac, w.est + 1 + (size_t)(tau + 1) * 4 * mm))) return rc;
        if (stable && tau + 1 < nmax) {
            if ((rc = k_itcf_propagate(h, w.B, psiR, psiR2))) return rc;
            std::swap(psiR, psiR2);
            if (tau != 0 && tau % nstblz == 0 && (rc = reortho_foreign(h, psiR, w.ot, w.detR))) return rc;
        }
    }
    // 4. FieldConfig.reset + copy_init_wfn: the next window starts from the walkers now
    if ((rc = window_end(h, true))) return rc;
    read_only.succeeded();
    if ((rc = copy_out(h, denom_out, w.est, sizeof(cplx)))) return rc;
    return copy_out(h, spgf_out, w.est + 1, sizeof(cplx) * nspgf);
}

// ---------------------------------------------------------------- energies of caller-supplied full Green's functions
int afq_local_energy_full_g(afq_handle *h, const double *G, int n, double *E_out) {
    if (!h || !G || !E_out || n < 1) return AFQ_EINVAL;
    if (h->kind != AFQ_SYS_GENERIC) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "full-G Cholesky energy: generic systems only");
    return full_g_call(h, G, n, E_out, 0, nullptr, [&](cplx *Gd, cplx *Ed, cplx *) { return k_energy_full_g(h, Gd, n, Ed); });
}

int afq_ueg_pair_sums(afq_handle *h, const double *G, int n, double *E_out, double *two_rdm_out) {
    if (!h || !G || !E_out || !two_rdm_out || n < 1) return AFQ_EINVAL;
    if (h->kind != AFQ_SYS_UEG) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "UEG pair sums: UEG systems only");
    return full_g_call(h, G, n, E_out, (size_t)4 * h->nq * n, two_rdm_out,
                       [&](cplx *Gd, cplx *Ed, cplx *Td) { return k_ueg_pair_sums(h, Gd, n, Ed, Td); });
}

int afq_correlations_full_g(afq_handle *h, const double *G, int n, double *corr_out) {
    if (!h || !G || !corr_out || n < 1) return AFQ_EINVAL;
    if (!h->kind) AFQ_FAIL(h, AFQ_ESTATE, "correlation functions: the system must be set (they are sized by its M)");
    return full_g_call(h, G, n, nullptr, (size_t)5 * h->M * h->M * n, corr_out,
                       [&](cplx *Gd, cplx *, cplx *Td) { return k_corr_full_g(h, Gd, n, Td); });
}

int afq_pairing_full_g(afq_handle *h, const double *G, int n, double *pair_out) {
    if (!h || !G || !pair_out || n < 1) return AFQ_EINVAL;
    if (!h->kind) AFQ_FAIL(h, AFQ_ESTATE, "pairing correlations: the system must be set (they are sized by its M)");
    if (!h->pair_nb) AFQ_FAIL(h, AFQ_ESTATE, "pairing correlations: no bond table (afq_set_pairing_bonds first)");
    return full_g_call(h, G, n, nullptr, (size_t)h->pair_nb * h->pair_nb * h->M * h->M * n, pair_out,
                       [&](cplx *Gd, cplx *, cplx *Td) { return k_pair_full_g(h, Gd, n, Td); });
}

int afq_hubbard_energy_full_g(afq_handle *h, const double *G, int n, double *E_out) {
    if (!h || !G || !E_out || n < 1) return AFQ_EINVAL;
    if (h->kind != AFQ_SYS_HUBBARD) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "full-G Hubbard energy: Hubbard systems only");
    return full_g_call(h, G, n, E_out, 0, nullptr, [&](cplx *Gd, cplx *Ed, cplx *) { return k_energy_hubbard_full_g(h, Gd, n, Ed); });
}

}  // extern "C"
