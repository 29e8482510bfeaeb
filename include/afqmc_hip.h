/*
 * afqmc_hip.h -- C ABI of libafqmc_hip.so: MI355X (gfx950) phaseless-AFQMC
 * walker propagation, Green's functions and local energies, walker-batched.
 *
 * The reference (pauxy-qmc/pauxy) has no FFI on this path: the hot path sits
 * behind the Python plug-in objects Propagator / Walkers / Estimators that
 * pauxy/qmc/afqmc.py drives.  Each entry point below therefore cites the
 * reference *Python* function it replaces (paths relative to the reference's
 * pauxy/ package); pauxy_amd/ holds the Python classes that bind these entry
 * points with ctypes behind the reference's own class/method names
 * (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - plain C: opaque handle, pointers, ints, doubles.  Every function returns
 *    0 (AFQ_OK) or a negative AFQ_E* code; afq_last_error() gives the text.
 *  - "c128" = complex128 as numpy stores it: interleaved (re, im) doubles,
 *    C order.  Host arrays are only read unless documented "out".
 *  - one handle per GPU, owned by one host thread; calls on one handle are
 *    serialised by the caller.  All work is queued on the handle's HIP stream;
 *    functions that return data to the host synchronise that stream first.
 *  - the handle owns every device allocation.
 */
#ifndef AFQMC_HIP_H
#define AFQMC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct afq_handle afq_handle;

#define AFQ_OK            0
#define AFQ_EINVAL       (-1)   /* bad argument                                  */
#define AFQ_ESTATE       (-2)   /* call order: system/trial/propagator/walkers   */
#define AFQ_EHIP         (-3)   /* HIP runtime error (text in afq_last_error)    */
#define AFQ_ENOMEM       (-4)
#define AFQ_EUNSUPPORTED (-5)
#define AFQ_EWEIGHT      (-6)   /* total weight < 1e-8 (walkers/handler.py:236)  */
#define AFQ_EOVERFLOW    (-7)   /* more walkers moved between two ranks in one population control than the
                                   exchange slots of the communicator hold (afq_comm_set_capacity)   */
#define AFQ_ECOMM        (-8)   /* communicator: a peer never signalled, probe mismatch, bootstrap failure */

/* system kinds */
#define AFQ_SYS_GENERIC 1
#define AFQ_SYS_HUBBARD 2
#define AFQ_SYS_UEG     3

/* propagator flags (propagation/continuous.py:18-37) */
#define AFQ_PROP_HYBRID          1   /* hybrid weight update (default)            */
#define AFQ_PROP_FORCE_BIAS      2
#define AFQ_PROP_FREE_PROJECTION 4
#define AFQ_PROP_HUBBARD_SPIN    8   /* charge_decomposition: false               */

/* walker fields for afq_walkers_set / afq_walkers_get.
 * per-walker shapes: PHI c128[M, na+nb]; WEIGHT, UNSCALED_WEIGHT, DETR f64;
 * OT, HYBRID_ENERGY, PHASE, ELOC c128; GHALF c128[na+nb, M] (alpha rows first);
 * G c128[2, M, M]; XBAR, XSHIFTED c128[K]; ENERGY c128[3]; LOG_DETR f64;
 * THERMAL_G f64[2, M, M], THERMAL_STACK f64[nbins, 2, M, M] (afq_thermal_configure) */
enum afq_field {
    AFQ_F_PHI = 0,
    AFQ_F_WEIGHT = 1,
    AFQ_F_UNSCALED_WEIGHT = 2,
    AFQ_F_OT = 3,
    AFQ_F_HYBRID_ENERGY = 4,
    AFQ_F_PHASE = 5,
    AFQ_F_DETR = 6,
    AFQ_F_ELOC = 7,
    AFQ_F_GHALF = 8,
    AFQ_F_G = 9,
    AFQ_F_XBAR = 10,
    AFQ_F_XSHIFTED = 11,
    AFQ_F_ENERGY = 12,
    AFQ_F_LOG_DETR = 13,
    AFQ_F_THERMAL_G = 14,       /* f64[2, M, M], thermal walkers (afq_thermal_configure); get and set      */
    AFQ_F_THERMAL_STACK = 15,   /* f64[nbins, 2, M, M], thermal walkers; get, and set for unit tests        */
    /* after afq_thermal_configure_continuous THERMAL_G and THERMAL_STACK are c128 of the same shapes, and there are: */
    AFQ_F_THERMAL_RIGHT = 16,   /* c128[2, M, M] product of the slices of the current bin                  */
    AFQ_F_THERMAL_M0 = 17,      /* c128[2] det G_s the next weight update divides by                        */
    AFQ_F_THERMAL_DET = 18,     /* c128[2] det G_s of the last Green's function evaluation (get only: a set is refused) */
    AFQ_F_CMF = 19,             /* c128: the mean-field and ...                                              */
    AFQ_F_CFB = 20,             /* ... force-bias factors of the last field kernel (get only: a set is refused) */
    AFQ_F_COUNT_
};

/* index of each accumulator in the estimates vector (estimators/mixed.py:460-469) */
enum afq_estimate {
    AFQ_EST_UWEIGHT = 0, AFQ_EST_WEIGHT = 1, AFQ_EST_ENUMER = 2, AFQ_EST_EDENOM = 3,
    AFQ_EST_EPROJ = 4, AFQ_EST_E1B = 5, AFQ_EST_E2B = 6, AFQ_EST_EHYB = 7,
    AFQ_EST_OVLP = 8, AFQ_EST_TIME = 9, AFQ_EST_COUNT_ = 10
};

/* ---- lifetime ----------------------------------------------------------- */
int afq_version(void);
int afq_create(int device_id, afq_handle **out);
int afq_destroy(afq_handle *h);
const char *afq_last_error(afq_handle *h);
int afq_sync(afq_handle *h);

/* ---- read-only inputs of the path --------------------------------------- */
/* systems/generic.py:74-166 arrays.  hs_pot f64[M*M, K] (= chol_vecs);
 * rchol c128[(na+nb)*M, K], row i*M+p, alpha block first
 * (trial_wavefunction/multi_slater.py:402-409); H1 c128[2,M,M].              */
int afq_set_system_generic(afq_handle *h, int M, int K, int na, int nb,
                           const double *hs_pot, const double *rchol,
                           const double *H1, double ecore);
/* The same system with complex Cholesky vectors (periodic / k-point Hamiltonians, complex orbitals;
 * pauxy/utils/io.py:200-206).  hs_pot c128[M*M, K], row p*M+q as above; the other arguments as
 * afq_set_system_generic.  The vectors are classified bitwise on upload: Hermitian
 * (L_n[q,p] == conj(L_n[p,q]) for every n) or general.  An hs_pot without imaginary parts takes the
 * real path (bitwise the results of afq_set_system_generic).  Back-propagation needs Hermitian
 * vectors: afq_bp_configure refuses general complex ones with AFQ_EUNSUPPORTED.                   */
int afq_set_system_generic_c128(afq_handle *h, int M, int K, int na, int nb,
                                const double *hs_pot, const double *rchol,
                                const double *H1, double ecore);
/* systems/hubbard.py:46-104.  T c128[2,M,M]; fields K = M.                    */
int afq_set_system_hubbard(afq_handle *h, int M, int na, int nb, double U,
                           const double *T);
/* systems/ueg.py:43-191,336-428.  iA, iB: CSC [M*M, nq] (colptr int64[nq+1],
 * rowidx int64[nnz], val c128[nnz]); the four ragged index lists of
 * systems/ueg.py:139-176 as offsets int64[nq+1] + flat int64 indices;
 * vqvec f64[nq]; H1diag f64[2,M]; fields K = 2*nq.                            */
int afq_set_system_ueg(afq_handle *h, int M, int nq, int na, int nb,
                       const int64_t *iA_colptr, const int64_t *iA_row, const double *iA_val,
                       const int64_t *iB_colptr, const int64_t *iB_row, const double *iB_val,
                       const int64_t *kpq_off, const int64_t *kpq_i, const int64_t *kpq_kpq,
                       const int64_t *pmq_off, const int64_t *pmq_i, const int64_t *pmq_pmq,
                       const double *vqvec, double vol, const double *H1diag, double ecore);
/* trial determinant psi c128[M, na+nb] (trial.psi after walkers/handler.py:61) */
int afq_set_trial(afq_handle *h, const double *psi);
/* ---- discrete Hirsch Hubbard-Stratonovich propagator -----------
 * propagation/hubbard.py:12-343 (Hirsch, single-site updates, constrained path) for a Hubbard system and a
 * single-determinant trial with N <= 128 electrons per spin (the inverse overlaps live in LDS up to N = 68 and are
 * updated in place in global memory beyond).  bt2 c128[2, M, M] = expm(-dt/2 T) (:36-37);
 * charge_decomposition selects the charge (complex gamma) or spin HS (:66-82).
 *   afq_propagate_hirsch   one step for every walker with |weight| > 1e-8, site uniforms from the device
 *                          Philox stream: kinetic + importance sampling (:148-172), M single-site
 *                          updates (:174-225), kinetic again, weight *= exp(dt eshift) (:285-312)
 *   afq_hirsch_kinetic / afq_hirsch_two_body / afq_hirsch_finish   the same step in three calls so that a
 *                          host driver can hand in numpy's uniforms: u f64[nw, M] (row w is read only if
 *                          walker w survived the first kinetic step, i.e. weight != 0 after it);
 *                          fields_out int32[nw, M] (chosen field 0/1, -1 not visited), used_out int32[nw]
 *                          (uniforms consumed; < M only when both field probabilities vanish) -- both
 *                          may be NULL.
 *   afq_hirsch_free_projection / afq_propagate_hirsch_free   propagate_walker_free (:303-343): no importance
 *                          sampling -- kinetic half step, every site takes field 0 (uniform < 0.5) or 1 and scales its row
 *                          of phi, kinetic half step, weight *= exp(dt eshift) |wfac|, phase *= exp(i arg wfac),
 *                          ot = <psi_T|phi>.  The first call switches the mode (the estimators then accumulate
 *                          weight * ot * phase, mixed.py:151-175, and the re-orthogonalisation folds det R into weight and
 *                          phase); u f64[nw, M] numpy's uniforms or NULL for the device stream, fields_out may be NULL.
 *   afq_hirsch_single_site    on = 0 replaces the M single-site updates of the three calls above (and of
 *                          afq_propagate_hirsch) by two_body_direct (:222-275, `single_site_update: False`): all M fields
 *                          drawn from the dynamic force bias of the current Green's function, phi scaled once, one overlap;
 *                          M uniforms per walker with a non-zero weight, no field history (back propagation: AFQ_EUNSUPPORTED). */
int afq_set_propagator_hirsch(afq_handle *h, const double *bt2, double dt, int charge_decomposition);
int afq_hirsch_free_projection(afq_handle *h, int on);
int afq_hirsch_single_site(afq_handle *h, int on);
int afq_propagate_hirsch_free(afq_handle *h, const double *u, int32_t *fields_out, double eshift);
int afq_propagate_hirsch(afq_handle *h, double eshift);
int afq_hirsch_kinetic(afq_handle *h);
int afq_hirsch_two_body(afq_handle *h, const double *u, int32_t *fields_out, int32_t *used_out);
int afq_hirsch_finish(afq_handle *h, double eshift);

/* Local energy of a generic Cholesky Hamiltonian from FULL Green's functions
 * (estimators/generic.py:398-434, local_energy_generic_cholesky; what estimators/mixed.py:383-437
 * dispatches to when no half-rotated Ghalf is given): G c128[n, 2, M, M] -> E c128[n, 3] = (E, E1b, E2b).
 * O(M^3 K) per Green's function; not on the per-step path.                                       */
int afq_local_energy_full_g(afq_handle *h, const double *G, int n, double *E_out);
/* The UEG energy's pair sums on FULL, general Green's functions, kept per momentum transfer (estimators/ueg.py:27-88,
 * local_energy_ueg(system, G, two_rdm=...)): G c128[n, 2, M, M] -> E c128[n, 3] = (E, E1b, E2b) without ecore (as
 * afq_local_energy on a UEG handle) and two_rdm c128[n, 2, 2, nq],
 *   two_rdm[s,s,q] = Gkpq[s,q] Gpmq[s,q] - Gprod[s,q],  two_rdm[s,t,q] = Gkpq[s,q] Gpmq[t,q] (s != t),
 * with the index lists the handle was given (any rows, any lengths, empty lists included); E2b = 1 / (2 vol) sum_q
 * vqvec[q] sum_st two_rdm[s,t,q].  Nothing is assumed about G (no zero rows).  Same input, same bits.  UEG handles
 * only (AFQ_EUNSUPPORTED); M < 65536.
 * afq_hubbard_energy_full_g: estimators/hubbard.py:93-114 on full Green's functions, ke = sum_s sum_ij T_s[i,j] G_s[i,j],
 * pe = U sum_i G_a[i,i] G_b[i,i]; Hubbard handles only.                                                        */
int afq_ueg_pair_sums(afq_handle *h, const double *G, int n, double *E_out, double *two_rdm_out);
int afq_hubbard_energy_full_g(afq_handle *h, const double *G, int n, double *E_out);
/* Density and spin correlation functions of FULL Green's functions by Wick's theorem for one pair of determinants
 * (k_corr.hip): G c128[n, 2, M, M] (spin 0 = up, 1 = down) -> corr c128[n, 5, M, M],
 *   corr[2s+t][i,j] = G_s[i,i] G_t[j,j]                                   (s != t)   <n_is n_jt>
 *   corr[2s+s][i,j] = G_s[i,i] G_s[j,j] + G_s[i,j] (d_ij - G_s[j,i])                 <n_is n_js>
 *   corr[4][i,j]    = G_0[i,j] (d_ij - G_1[j,i])                                     <S+_i S-_j> for G[i,j] = <c+_i c_j>
 * Slices 0-3 are the same for G and for its transpose per spin; slice 4 is transposed with G.  Nothing is assumed
 * about G.  Any handle whose system is set (AFQ_ESTATE before that): only M is used.  Same input, same bits.       */
int afq_correlations_full_g(afq_handle *h, const double *G, int n, double *corr_out);
/* Pair-field correlation functions of FULL Green's functions over a table of bonds (k_pair.hip).
 * afq_set_pairing_bonds: nbr int32[nb, M], nbr[b][i] = the partner site of i along bond b, or -1 where i has no such
 * partner (open boundaries, Generic systems); any table, repeated partners included.  Needs a system (AFQ_ESTATE before
 * that; a new system drops the table); nb <= 16 (AFQ_EINVAL above, with the number) and every entry in [-1, M)
 * (AFQ_EINVAL naming the entry; the table held before stays).  nb = 0 clears the table (nbr may be NULL then).  A window
 * in the mode of afq_bp_pairing leaves that mode: call afq_bp_pairing again after a new table.
 * afq_pairing_full_g: G c128[n, 2, M, M] (spin 0 = up, 1 = down) -> pair c128[n, nb, nb, M, M].  With
 * D+(k, l) = c+_k,up c+_l,down and G[i,j] = <c+_i c_j>,
 *   pair[b, b', i, j] = <D+(i, nbr[b][i]) D(j, nbr[b'][j])> = G_0[i, j] G_1[nbr[b][i], nbr[b'][j]],
 * Wick's theorem for one pair of determinants (opposite spins: no exchange term), and 0 where either partner is -1
 * whatever G holds.  For the transposed convention (the back-propagated G is the transpose) the array comes out with
 * both index pairs exchanged: its element [b, b', i, j] is pair[b', b, j, i] of the definition above.  Nothing is
 * assumed about G.  Any handle with a system and a bond table (AFQ_ESTATE without either).  Same input, same bits.  */
int afq_set_pairing_bonds(afq_handle *h, int nb, const int32_t *nbr);
int afq_pairing_full_g(afq_handle *h, const double *G, int n, double *pair_out);

/* ---- back-propagated estimator --------------------------------
 * estimators/back_propagation.py:63-226, walkers/stack.py:5-127 (FieldConfig),
 * propagation/generic.py:181-211,253-290.  After afq_bp_configure every
 * afq_propagate records the shifted fields x - xbar of each walker together with
 * the phase / cosine factors of the weight update (up to nbp steps; the history,
 * phi_old and the factors travel with the walker through the comb, afq_walkers_copy
 * and afq_walker_pack / unpack).  Call after afq_walkers_alloc and afq_set_propagator;
 * phi_old starts as the current phi.
 * Hubbard systems: with the discrete Hirsch propagator the kernel of afq_hirsch_two_body / afq_propagate_hirsch
 * records the chosen field of every site as it goes (FieldConfig.push, walkers/stack.py:35-49, called at
 * propagation/hubbard.py:215-216; no weight factors on this path), and afq_bp_update applies
 * B(x)^H = (BT2 diag(auxf[x, spin]) BT2)^H of propagation/hubbard.py:568-600,634-672; the continuous Hubbard
 * propagator is refused (the reference would read its fields as 0 / 1 indices, estimators/back_propagation.py:125). */
int afq_bp_configure(afq_handle *h, int nbp);
/* FieldConfig.step of every walker: int32[nw]                                   */
int afq_bp_steps(afq_handle *h, int32_t *steps_out);
/* BackPropagation.update_uhf for the whole population: back-propagates phi_bp0
 * (trial.psi or trial.init, c128[M, na+nb]) through every walker's recorded fields
 * (most recent first, re-orthogonalised every nstblz steps), forms
 * G_bp[w] = gab(phi_bp, phi_old)^T and returns est_out c128[4 + 2 M M] =
 * [0, 0, 0, sum_w wt_w, sum_w wt_w G_bp[w]] with wt = weight (restore_weights 0),
 * weight * prod(I/|I|) (1, "partial") or weight * prod(I/|I|) / prod(cos) (2, "full");
 * then, when `reset` is set (the last of the nsplit path lengths, back_propagation.py:68-69,219-222), resets the
 * histories and copies phi -> phi_old.  Generic systems (propagation/generic.py:253-290) and the UEG
 * (propagation/planewave.py:114-178; B(x)^H = B(-conj x) for both).  With eval_energy the entries 0-2 are
 * sum_w wt_w (E, E1b, E2b)[G_bp[w]]: the full-G Cholesky energy (generic systems), local_energy_hubbard on G_bp
 * (Hubbard, discrete fields), the pair sums of afq_ueg_pair_sums on G_bp (UEG; ecore not included).            */
int afq_bp_update(afq_handle *h, const double *phi_bp0, int nstblz, int restore_weights, int eval_energy,
                  int reset, double *est_out);
/* Back-propagated two-body RDM and extended Koopmans' theorem (EKT) Fock matrices (estimators/back_propagation.py:
 * 168-175,178-186, estimators/ekt.py:10-73).  Call after afq_bp_configure; says what afq_bp_update_ext may be asked for.
 *   two_rdm  spin-summed two_rdm[p,r,q,s] = S[p,r] S[q,s] - sum_s G_s[p,s] G_s[q,r], S = G_a + G_b (layout [p][r][q][s]).
 *            AFQ_ENOMEM (with the byte count) when its 16 M^4 bytes exceed half of the free device memory.
 *   ekt      F1p / F1h of ekt_1p_fock_opt / ekt_1h_fock_opt with h1 c128[M, M] and the vectors L c128[nL, M, M]:
 *            the UEG passes 2 chol_vecs^T reshaped (nL = nq); generic systems pass L = NULL (nL = K) for their own
 *            vectors, L_x[i,k] = hs_pot[i*M+k, x] (the reference's ekt.py refuses the [M*M, K] layout of a Generic
 *            system; this is its function applied to that reshape).  AFQ_EUNSUPPORTED on Hubbard systems and for
 *            L = NULL with complex vectors (afq_set_system_generic_c128).
 * The hot path is k_bp_obs.hip: the EKT quadratic terms in rank-N form from the factors of G_bp (phi_bp and the
 * half-rotated G_bp), the terms linear in G once per window on sum_w wt_w G_bp[w]; the two-body RDM as one MFMA GEMM
 * per (p, q) over the stacked walker contraction.
 *   two_rdm = 2  (UEG handles only, AFQ_EUNSUPPORTED elsewhere) the structure factor instead: afq_bp_update_ext's
 *            two_rdm_out then is c128[2, 2, nq] = sum_w wt_w two_rdm[G_bp[w]] of afq_ueg_pair_sums, walkers summed in
 *            index order (no atomics: the same bits on every run); walkers of weight zero contribute nothing.
 *            Evaluated with or without eval_energy.
 *   two_rdm = 3  (every system, also together with ekt) the correlation functions instead: two_rdm_out then is
 *            c128[5, M, M] = sum_w wt_w corr[G_bp[w]] of afq_correlations_full_g, O(M^2) where the two-body RDM is
 *            O(M^4): no memory check.  Walkers are summed in index order in chunks of a fixed length, the chunks in
 *            chunk order (no atomics: the same bits on every run and every device); walkers of weight zero contribute
 *            nothing.  Evaluated with or without eval_energy.                                          */
int afq_bp_observables(afq_handle *h, int two_rdm, int ekt, const double *h1, const double *L, int nL);
/* Puts the window's two-body slot into pairing mode (on != 0) or takes it out of it (on = 0; a slot in another mode is
 * left as it is).  Call after afq_bp_configure (AFQ_ESTATE before) and afq_set_pairing_bonds (AFQ_ESTATE without a
 * table).  afq_bp_update_ext's two_rdm_out then is c128[nb, nb, M, M] = sum_w wt_w pair[G_bp[w]] of afq_pairing_full_g
 * (G_bp is the transposed convention: see there), with the wt_w of the one-body sum; walkers are summed in index order
 * in chunks of a fixed length, the chunks in chunk order (no atomics: the same bits on every run and every device),
 * walkers of weight zero contribute nothing.  Evaluated with or without eval_energy; what afq_bp_observables set for
 * the EKT stays and works alongside.  A later afq_bp_observables replaces the mode with its own.  Every system;
 * AFQ_EUNSUPPORTED with a multi-determinant trial.                                                    */
int afq_bp_pairing(afq_handle *h, int on);
/* afq_bp_update plus, where the pointers are not NULL, two_rdm_out c128[M^4] (c128[2, 2, nq] / c128[5, M, M] in the
 * modes 2 / 3 of afq_bp_observables, c128[nb, nb, M, M] after afq_bp_pairing) = sum_w wt_w two_rdm[G_bp[w]] and
 * fock_out c128[2, M, M] = sum_w wt_w (F1p, F1h)[G_bp[w]] with the weights of est_out (complex with restore_weights).
 * With both NULL it is afq_bp_update, bitwise.                                                       */
/* Cholesky vectors per chunk of the EKT: nc for the rank-N panels, ncy for the term linear in G (0 = automatic: as
 * many as fit 1 GiB of scratch, independent of the free memory, so that the order of the sums is reproducible). */
int afq_bp_ekt_chunks(afq_handle *h, int nc, int ncy);
int afq_bp_update_ext(afq_handle *h, const double *phi_bp0, int nstblz, int restore_weights, int eval_energy,
                      int reset, double *est_out, double *two_rdm_out, double *fock_out);
/* The window of a multi-determinant trial |psi_T> = sum_d c_d |D_d> (afq_set_trial_multi; generic systems).  On such a
 * handle afq_bp_configure sizes phi_bp for ndet determinants per walker and the window's scratch, and refuses with
 * AFQ_ENOMEM (and the byte counts) when they exceed half of the free device memory.  The reference has no such window
 * (its BackPropagation fails on ndets > 1); what is computed, per walker over its recorded fields x_1 .. x_n:
 *   1. D_d^bp = B(x_1)^H .. B(x_n)^H D_d for every determinant, the operator and the re-orthogonalisation schedule of
 *      afq_bp_update; the HS potential of a backward step is built once per walker, not once per determinant, and on
 *      the GEMM chain the ndet determinants of a walker are one column-stacked operand [M, ndet (na+nb)].
 *   2. A re-orthogonalisation replaces D by Q with D = Q R, diag R > 0.  With one determinant det R cancels between
 *      numerator and denominator; with several it does not: log r_d = sum of log det R_alpha + log det R_beta over
 *      the re-orthogonalisations is kept per (walker, d), and
 *        w_d = conj(c_d) exp(log r_d - max_d' log r_d') det(Q_d,alpha^H phi_old,alpha) det(Q_d,beta^H phi_old,beta);
 *      a w_d that is zero or not finite counts as zero, and a walker whose sum_d w_d is zero or not finite does not
 *      contribute to numerator or denominator.
 *   3. G_d = gab(Q_d, phi_old)^T per spin, G_bp[w] = sum_d w_d G_d / sum_d w_d.
 *   4. est_out as afq_bp_update's: [E, E1b, E2b sums, sum_w wt_w, sum_w wt_w G_bp[w]] with the same wt_w; with
 *      eval_energy E_w = sum_d w_d E[G_d] / sum_d w_d from the full-G Cholesky energy of every G_d (not E[G_bp]: the
 *      two-body part is quadratic in G).
 * dets c128[ndet, M, na+nb], coeffs c128[ndet]; ndet must be the handle's.  detw_out (may be NULL) c128[nw, ndet]:
 * w_d / sum_d w_d per walker, the counterpart of afq_walkers_det_weights.  The window is read-only on the walk like
 * afq_itcf_update's (its Green's functions live in its own scratch).  afq_bp_update on such a handle is the
 * single-determinant window of phi_bp0 (init_walker).  AFQ_EUNSUPPORTED with a multi-determinant trial:
 * afq_bp_observables (two-body RDM, EKT) and afq_itcf_configure.                                       */
int afq_bp_update_msd(afq_handle *h, int ndet, const double *dets, const double *coeffs, int nstblz, int restore_weights,
                      int eval_energy, int reset, double *est_out, double *detw_out);

/* Imaginary-time single-particle Green's function (the ITCF estimator, estimators/itcf.py of the reference).
 * afq_itcf_configure: windows of n = nmax + neqlb steps (nmax >= 1, neqlb >= 0); sizes the field history of
 * afq_bp_configure to n (a history of another length configured before: AFQ_ESTATE), which comb, copy and pack carry
 * as for back-propagation.  stable: 1 the Feldbacher-Assaad chain, 0 the plain products; restore_weights: 1 weighs a
 * walker by weight * (phase product / cosine product) of the window, 0 by its weight.
 * AFQ_EUNSUPPORTED: M > 128, plane-wave (UEG) systems, continuous Hubbard fields, multi-determinant trials, general
 * complex Cholesky vectors, restore_weights with discrete fields, free projection.
 * afq_itcf_update: one window over the recorded history and the trial psi_T c128[M, na+nb] (the window's left end):
 *   B_t = BT2 E(x_t) BT2 (E the order-6 Taylor exponential of the VHS, or diag(auxf) for discrete fields),
 *   psi_R(0) the walkers at the window start, psi_R(t+1) = B_t psi_R(t); psi_L(n) = psi_T, psi_L(t) = B_t^H psi_L(t+1);
 *   both re-orthogonalised every nstblz steps; P(t) = gab(psi_L(t), psi_R(t)) per spin;
 *   stable: Ggr(t+1) = B_t (I - P(t)) Ggr(t), Gls(t+1) = Gls(t) P(t) B_t^-1 from Ggr(0) = I - P(0), Gls(0) = P(0);
 *   unstable: Ggr(t+1) = B_t Ggr(t), Gls(t+1) = Gls(t) B_t^-1;
 *   spgf_out c128[nmax+1][2 spin][2: greater, lesser][M][M] = sum_w wfac_w Re G_w(t), denom_out c128 = sum_w wfac_w
 *   (walkers without a complete window count 0).  Then the history restarts and the window start is the walkers now.
 *   The window is read-only on the walk: walkers, weights, overlaps, the cached Green's function the last step left
 *   for the next one (Ghalf) and the full G the mixed one_rdm accumulates are what they were (the window's own Green's
 *   functions live in its scratch), so a run with windows is bitwise the run without them.
 * AFQ_ESTATE before afq_itcf_configure; AFQ_ENOMEM when the stored psi_L
 * (16 nw nmax M (na+nb) bytes) exceed half of the free device memory.                                 */
int afq_itcf_configure(afq_handle *h, int nmax, int neqlb, int stable, int restore_weights);
int afq_itcf_update(afq_handle *h, const double *psi_T, int nstblz, double *spgf_out, double *denom_out);

/* Multi-determinant (NOMSD / PHMSD) trial |psi_T> = sum_d c_d |D_d> for a generic system, replacing
 * the single-determinant operands of afq_set_system_generic / afq_set_trial.  Call after the
 * system and before afq_walkers_alloc.
 *   psi    [ndet, M, na+nb] c128     pauxy/trial_wavefunction/multi_slater.py:36-38 (trial.psi)
 *   coeffs [ndet] c128               trial.coeffs (enter as conj(c_d), walkers/multi_det.py:226)
 *   rchol  [ndet, (na+nb) M, K] c128 per-determinant half rotation, multi_slater.py:370-409
 * Green's function / overlap, force bias and local energy then follow walkers/multi_det.py:194-257,
 * 135-162, propagation/generic.py:154-157 and estimators/mixed.py:439-448 (the per-determinant
 * energy is evaluated in its half-rotated form, algebraically equal to the reference's full-G form). */
int afq_set_trial_multi(afq_handle *h, int ndet, const double *psi, const double *coeffs, const double *rchol);
/* weights conj(c_d) <D_d|phi_w> of the last Green's function / overlap evaluation: [nw, ndet] c128
 * (MultiDetWalker.weights, walkers/multi_det.py:226)                                                  */
int afq_walkers_det_weights(afq_handle *h, double *weights_out);

/* propagation/continuous.py:13-80 + <system>.construct_one_body_propagator:
 * BH1 c128[2,M,M], mf_shift c128[K], dt, expansion_order, AFQ_PROP_* flags.    */
int afq_set_propagator(afq_handle *h, const double *BH1, const double *mf_shift,
                       double dt, int exp_order, int flags);

/* ---- walker population (walkers/handler.py:36-164, walkers/walker.py:24-61) */
int afq_walkers_alloc(afq_handle *h, int nw);
int afq_walkers_set(afq_handle *h, int field, const void *host, int first, int count);
int afq_walkers_get(afq_handle *h, int field, void *host, int first, int count);
/* device pointer of a field (row `first`), for zero-copy plumbing */
int afq_walkers_device_ptr(afq_handle *h, int field, void **dev_ptr, int64_t *bytes_per_walker);

/* ---- the hot path -------------------------------------------------------- */
/* walkers/single_det.py:295-321 for every walker: Ghalf (+ full G when
 * want_G or the system needs it) and det(phi^T psi*) -> ovlp_out c128[nw]
 * (may be NULL).                                                            */
int afq_greens(afq_handle *h, int want_G, double *ovlp_out);
/* walkers/single_det.py:170-199 for every walker -> ovlp_out c128[nw]         */
int afq_calc_overlap(afq_handle *h, double *ovlp_out);
/* O^-1 of every walker and spin, O = phi_s^T conj(psi_s) (so O^-1 = inv_O of estimators/greens_function.py:82-115
 * and the transpose of SingleDetWalker.inv_ovlp, walkers/single_det.py:95-115): c128[nw, 2, nmax, nmax] row-major with
 * leading dimension nmax = max(na, nb), zero padded; ovlp_out c128[nw] may be NULL.  N <= 128.                         */
int afq_inverse_overlap(afq_handle *h, double *oinv_out, double *ovlp_out);
/* propagation/continuous.py:232-262 (phaseless) or :175-200 (free projection)
 * for every live walker (|weight| > 1e-8, qmc/afqmc.py:232).
 * xi: host f64[nw, K] normal fields (row iw used only if walker iw is live),
 * or NULL to draw them on the device (afq_rng_seed).                         */
int afq_propagate(afq_handle *h, const double *xi, double eshift_re, double eshift_im);
/* The same step in two calls.  Only the weight update at the very end of a step reads the energy shift
 * (propagation/continuous.py:194-200, :206-230): afq_propagate_begin enqueues everything up to and including the
 * propagation of the Slater matrices, afq_propagate_finish the overlap / Green's function of the propagated walkers and
 * the weight update.  A driver that derives the shift of the next block from the estimators of the block just ended
 * (qmc/afqmc.py:247-250 after estimators/mixed.py:261-273) can therefore enqueue the first part of the next step BEFORE
 * it waits for those estimators (afq_estimates_get_begin / _end below) and keep the device busy across the block
 * boundary.  afq_propagate(h, xi, e) == afq_propagate_begin(h, xi) + afq_propagate_finish(h, e); between the two calls
 * only afq_estimates_get_end, afq_set_weight_cap and afq_last_error may be called (AFQ_ESTATE otherwise).           */
int afq_propagate_begin(afq_handle *h, const double *xi);
int afq_propagate_finish(afq_handle *h, double eshift_re, double eshift_im);
/* walkers/handler.py:166-181 -> walkers/single_det.py:215-255; detR f64[nw] out (may be NULL) */
int afq_reortho(afq_handle *h, double *detR_out);
/* walkers: {use_log_shift: true} (walkers/handler.py:45,228,456-475, walkers/single_det.py:159,192,250-253,320).
 * Every walker carries the same log_shift / detR_shift (walker.py:49-52, handler.py:471-474), so they are handle
 * state: walker.ot = overlap * exp(-log_shift) on the continuous path (exp(+log_shift) behind calc_otrial on the
 * discrete path, :159), detR = exp(log det R - detR_shift), and AFQ_F_LOG_DETR accumulates log(detR) per walker.
 * on == 0 switches the option off.  afq_calc_overlap / afq_greens keep returning the unshifted determinant.
 * afq_log_ovlp_sums: f64[3] = sums over this rank's walkers of |ot|, |detR|, |log_detR| (handler.py:457-462);
 * the caller reduces them over ranks and feeds the running averages back through afq_set_log_shift.          */
int afq_set_log_shift(afq_handle *h, int on, double log_shift, double detR_shift);
int afq_log_ovlp_sums(afq_handle *h, double *sums3);
/* estimators/mixed.py:383-437 dispatch for every walker, from the current
 * Ghalf/G (call afq_greens first): E c128[nw,3] = (E, E1, E2); may be NULL.   */
int afq_local_energy(afq_handle *h, double *E_out);

/* The exchange part of estimators/generic.py:198-216 has two device algorithms with the same result:
 *   1  T-intermediate: T[x,i,j] = sum_p rchol[(i,p),x] Ghalf[j,p] on MFMA tiles, traced in registers
 *      (4 K M N^2 flops per spin and walker)
 *   2  quadratic form: exx = g^T Atil g with Atil[(j,p),(i,q)] = sum_x rchol[(i,p),x] rchol[(j,q),x] built once per
 *      trial ((N M)^2 entries per spin in HBM) -- one [nw x NM] x [NM x NM] GEMM per evaluation, K / M times
 *      fewer flops
 * mode 0 (default) picks 2 when K >= M and the operands of all determinants fit 72 GB, else 1.            */
int afq_set_exchange_algorithm(afq_handle *h, int mode);
int afq_exchange_algorithm(afq_handle *h, int *mode_out);

/* A closed-shell walker (spin blocks bitwise equal, found by the fused propagator on the walker itself at every launch)
 * has two forms of its propagation with the same result to rounding:
 *   1  streamed deal: the Taylor products of the alpha half, V streamed through the LDS operand ring for every product
 *   2  resident body: V loaded once per walker and step into registers as MFMA A fragments, no ring in the products;
 *      exists for one real one-body matrix for both spins, na == nb in 17 .. 32, 96 < M <= 104, exp_order > 0
 * mode 0 (default) picks 2 where it exists; mode 2 on any other shape runs 1.  The getter reports the form closed
 * walkers take with the handle's present shape and setting.                                                        */
int afq_set_propagator_closed_form(afq_handle *h, int mode);
int afq_propagator_closed_form(afq_handle *h, int *mode_out);

/* A step announced with afq_estimates_fuse_next and run by afq_propagate (begin and finish in one call) ends in a Green's
 * function of which only the overlaps and the spin sum of Ghalf are kept.  In the shape class of the resident closed-shell
 * propagator (above; single determinant, hybrid weights with force bias, no back-propagation window, no RDM) that evaluation,
 * with the weight update, runs as the tail of the propagator's own launch:
 *   0  never: two launches, as every other step
 *   1  tail behind the propagator as it is (4-multiplication Taylor products): the same bits as mode 0
 *   2  (default) tail behind the resident body with 3-multiplication Taylor products: the same result to rounding      */
int afq_set_step_fusion(afq_handle *h, int mode);
/* Which steps of that shape class run the tail (modes 1 and 2 keep their meaning: the body behind which it runs):
 *   0  (default) announced steps run by afq_propagate only
 *   1  every afq_propagate and afq_propagate_begin.  An unannounced step's tail stores the per-spin Ghalf as well; the
 *      tail of afq_propagate_begin, which does not know the energy shift, leaves the weight update to
 *      afq_propagate_finish (one weight_kernel launch).
 * AFQ_EINVAL for any other value.                                                                                   */
int afq_set_step_fusion_scope(afq_handle *h, int scope);
/* Mode 2's launch, for the walkers of the resident body (single real closed trial, which that tail's one-spin path needs
 * anyway): with psi^H B made once per upload of the trial or the propagator, the tail's overlap matrix is (psi^H B) S -- S the
 * Taylor sum the last product leaves in LDS --: the eight waves multiply it ahead of the closing one-body pass, one wave
 * inverts it while the others run that pass, and the tail starts at O^-1 phi^T.  The overlap matrix is rounded as (psi^H B) S instead of psi^H (B S): overlaps,
 * weights and Ghalf of those walkers move at rounding level.
 *   1  (default) on      0  off: the launch of before, bit for bit
 * Modes 0 and 1, and every walker that does not take the resident body, are not touched.  afq_counters_ext [8] counts the
 * walker steps that took it.  AFQ_EINVAL for any other value.                                                       */
int afq_set_step_tail_overlap(afq_handle *h, int on);
/* The step hand-over of that launch (mode 2 with the early overlap, same walkers): under the inversion the idle waves also
 * make the opening one-body pass of the NEXT step, T_0 = B phi' = (B B) S with B B made on the host once per upload of the
 * propagator, and leave it in a per-walker buffer of the handle; the next launch of the kernel starts such a walker at its
 * Taylor products and reads no phi.  The handle drops the hand-over whenever anything comes between the two launches that
 * writes phi or moves a walker to another slot (re-orthogonalisation, population control, copy, unpack, exchange, upload,
 * a window), changes the propagator, the trial or one of the step's mode switches, or launches any other propagator; the
 * next step then runs its own opening pass.  T_0 is rounded as (B B) S instead of B (B S): results move at rounding level.
 *   1  (default) on      0  off: the launch of before
 * afq_counters_ext [9] counts the walker steps that started from a hand-over.  AFQ_EINVAL for any other value.        */
int afq_set_step_handover(afq_handle *h, int on);

/* Force bias of a multi-determinant trial (propagation/generic.py:154-157, walkers/multi_det.py:283-290) has two
 * device algorithms with the same result:
 *   1  one half-rotated contraction per determinant, rchol_d^T vec(Ghalf_d), averaged with the weights
 *      conj(c_d) <D_d|phi> afterwards (ndet, or 2 ndet for complex vectors, times K (Na + Nb) M products)
 *   2  the reference's own formulation: the weights go into ONE determinant-averaged Green's function
 *      Gbar = sum_d w_d conj(psi_d) Ghalf_d / sum_d w_d, contracted once with the symmetric-packed hs_pot
 *      (K M (M + 1) / 2 products + the build of Gbar); needs symmetric real or Hermitian complex L_n (general complex
 *      L_n always run mode 1, whatever is asked for)
 * mode 0 (default) picks 2 when it is the cheaper one for more than 32 walkers.  afq_msd_force_bias: what the next
 * force bias will use (0 for a single-determinant trial).                                                          */
int afq_set_msd_force_bias(afq_handle *h, int mode);
int afq_msd_force_bias(afq_handle *h, int *mode_out);

/* unit-test hooks (reference: <system propagator>.construct_force_bias /
 * construct_VHS, Continuous.apply_exponential, operations.kinetic_real)       */
int afq_force_bias(afq_handle *h, double *xbar_out);                 /* c128[nw,K] */
int afq_shift_fields(afq_handle *h, const double *xi, const double *xbar,
                     double *xs_out, double *cmf_out, double *cfb_out); /* continuous.py:140-158 */
int afq_vhs(afq_handle *h, const double *xs, double *vhs_out);       /* c128[nw,nv,M,M] */
int afq_vhs_count(afq_handle *h, int *nv);                           /* 1, or 2 for spin HS */
int afq_apply_exponential(afq_handle *h, const double *vhs);         /* phi <- Taylor(vhs) phi */
int afq_kinetic(afq_handle *h);                                      /* phi <- BH1 phi */

/* ---- driver glue that must stay on the device between steps --------------- */
/* qmc/afqmc.py:235-236: weight > frac*total_weight -> frac*total_weight.  A negative
 * total_weight means "the total weight the last afq_popcontrol_comb measured" (kept on the
 * device; the population size before the first comb), which needs no host round trip.     */
int afq_cap_weights(afq_handle *h, double frac, double total_weight);
/* The same cap applied by afq_propagate itself, at the end of its weight-update kernel (one launch
 * less per step).  frac <= 0 switches it off (the default); total_weight as in afq_cap_weights.   */
int afq_set_weight_cap(afq_handle *h, double frac, double total_weight);
/* walkers/handler.py:225-338 for a single rank: rescale, comb with the uniform
 * r, clone/kill, weights reset to 1.  parent_ix int32[nw] out (may be NULL);
 * total_weight_out f64 (may be NULL).  With BOTH outputs NULL the call only enqueues
 * work (no host synchronisation, no AFQ_EWEIGHT check).                         */
int afq_popcontrol_comb(afq_handle *h, double r, double target_weight,
                        int32_t *parent_ix, double *total_weight_out);
/* walkers/handler.py:225-251,340-412 for a single rank (population_control: pair_branch): rescale as the comb does;
 * order the walkers by |weight| (stable); pair the p-th lightest with the p-th heaviest and act on the pair while its
 * light walker is below min_weight or its heavy one above max_weight (the first pair that is neither ends it); pair p
 * uses u[p]: with probability a_heavy / (a_light + a_heavy) the heavy walker is cloned, else the light one, and both
 * copies carry half the pair's weight.  The j-th clone by index overwrites the j-th kill by index.  Walkers outside a
 * pair keep their scaled, signed weight; nothing is reset to 1 and the total weight is conserved.
 *   u       nu >= nw / 2 uniforms on the host (AFQ_EINVAL below that); staged by the call, the caller may free them
 *   mult    int32[nw] out (may be NULL): 0 kill, 1 keep, 2 clone
 *   ndraws_out (may be NULL) how many uniforms were consumed: u[0 .. ndraws)
 *   total_weight_out (may be NULL) the total weight before scaling, what afq_cap_weights(.., -1) then uses
 * With all three outputs NULL the call only enqueues work (no host synchronisation, no AFQ_EWEIGHT check); a collapsed
 * population (total < 1e-8) changes nothing and is reported by the next synchronising call, as for the comb.
 * One work-group plans in LDS: at most AFQ_PAIR_BRANCH_MAX_WALKERS walkers (AFQ_EUNSUPPORTED above).  With a
 * library-owned communicator of more than one rank attached: AFQ_EUNSUPPORTED (that communicator does the comb only;
 * with a one-rank communicator the call is the single-rank event).                                                   */
#define AFQ_PAIR_BRANCH_MAX_WALKERS 8192
int afq_popcontrol_pair_branch(afq_handle *h, const double *u, int nu, double target_weight,
                               double min_weight, double max_weight, int32_t *mult,
                               int32_t *ndraws_out, double *total_weight_out);

/* ---- library-owned communicator ----------------------------------------------------
 * walkers/handler.py:225-338 across ranks -- the Allgather of the weights (:232), rank 0's comb uniform
 * (:276,291) and the point-to-point walker copies (:303-331) -- and the estimator reduction of
 * estimators/mixed.py:261,273, on the device over RCCL (xGMI on one node), one process per GPU.
 * After afq_comm_init, afq_popcontrol_comb is a collective: every rank calls it with the same
 * target_weight (= total walkers) and rank 0's r; the weights are all-gathered on the device, every rank
 * decides the identical global comb, cloned walkers that change rank are written by the sending GPU straight
 * into the receiving GPU's mapped window (live slots only), nothing is read back by the host unless outputs are requested
 * (parent_ix is then the GLOBAL int32[nranks * nw] comb, total_weight_out the global weight).  The cap of
 * afq_cap_weights / afq_set_weight_cap with total_weight < 0 uses the global weight of the last comb.
 *   afq_comm_unique_id     128-byte ncclUniqueId, made by rank 0 and handed to every rank by the caller
 *   afq_comm_available     1 if librccl can be loaded in this process (no collective: lets the ranks AGREE on calling
 *                          afq_comm_init before any of them blocks inside ncclCommInitRank)
 *   afq_comm_init          ncclCommInitRank on the handle's GPU (librccl is loaded here, not before)
 *   afq_comm_init_ipc      the same communicator without RCCL: every rank maps every peer's window
 *                          (hipIpcGetMemHandle / hipIpcOpenMemHandle, xGMI peer access on one node) and all three
 *                          exchanges -- weights all-gather, walker slots, estimator reduction -- are kernels writing
 *                          into the peers' windows, ordered by system-scope flags.  `allgather(send, recv, bytes, user)`
 *                          is the caller's all-gather of `bytes` per rank over its own communicator (MPI /
 *                          torch.distributed; returns 0): the bootstrap for the window handles, called on the host at
 *                          afq_comm_init_ipc time and whenever the windows are re-made (first population control,
 *                          capacity change) -- at the same call on every rank
 *   afq_comm_set_transport 1 (default): walkers that change rank are written by the pack kernel straight into the
 *                          destination rank's mapped window, LIVE SLOTS ONLY, no host knowledge of the counts, nothing
 *                          posted by the host; 0 (RCCL communicator only; also the automatic fall-back when a rank cannot
 *                          export / map windows): fixed-capacity slots to and from every peer in one ncclSend / ncclRecv group
 *   afq_comm_set_capacity  walkers one rank can send to one peer per event (default nw up to 512 walkers per rank:
 *                          what a rank owns, cannot overflow; max(512, nw / 4) above, so that the windows stay a few
 *                          hundred MB); exceeding it raises AFQ_EOVERFLOW at the next afq_estimates_get / fetching comb.
 *                          Only the ncclSend / ncclRecv transport pays link time for unused capacity
 *   afq_comm_set_timeout   how long (seconds, > 0) a kernel waits for a peer before it gives up; default 300 s, or
 *                          AFQ_COMM_TIMEOUT_S from the environment when a communicator is created.  The budget covers
 *                          whatever may delay one rank between two collectives (rank 0 writing output or restart files,
 *                          a file-system stall, first-use code loading); it is per process and GPU, not per handle
 *   afq_comm_probe         collective known-answer round through the all-gather, one full slot to and from every peer on
 *                          the configured transport, and the all-reduce; AFQ_ECOMM on any mismatch
 *                          (mismatch_out int64[3], may be NULL: collective values, slot elements, flags that never came)
 *   afq_comm_stats         int64[AFQ_COMM_NSTATS]: largest per-peer transfer seen, events, capacity, overflow flag, rank,
 *                          size, walkers sent, bytes sent, transport (1 windows / 0 send-recv), communication error flag,
 *                          communicator kind (0 in-process, 1 RCCL, 2 IPC), window memory kind (1 uncached,
 *                          2 fine-grained, 3 plain)
 *   afq_estimates_allreduce  sum over ranks of buf c128[nest] (in/out, host), or with buf == NULL of the
 *                          device accumulators of afq_estimates_update in place (no host round trip; a
 *                          following afq_estimates_get returns the global sums on every rank)
 * A kernel that waits for a peer gives up after the wait budget and raises a sticky error, reported as AFQ_ECOMM by
 * the next synchronising call (afq_estimates_get / _end, a fetching afq_popcontrol_comb) -- never a hung device.  The
 * sticky flags and statistics belong to the communicator: creating or destroying one clears them.
 * In-process variant: afq_comm_init_local makes handles[0..n) (one host thread driving several GPUs, or
 * several handles on one GPU) the ranks 0..n-1 of one communicator; the collectives are then the group calls
 * afq_popcontrol_comb_local / afq_estimates_allreduce_local (the kernels and windows of the IPC communicator, the
 * windows being plain device pointers of the one process).                                               */
#define AFQ_COMM_ID_BYTES 128
#define AFQ_COMM_NSTATS 12
typedef int (*afq_allgather_fn)(const void *send, void *recv, int bytes, void *user);
int afq_comm_unique_id(void *id_out);
int afq_comm_available(void);
int afq_comm_init(afq_handle *h, const void *unique_id, int rank, int nranks);
int afq_comm_init_ipc(afq_handle *h, int rank, int nranks, afq_allgather_fn allgather, void *user);
int afq_comm_destroy(afq_handle *h);
int afq_comm_set_transport(afq_handle *h, int window);
int afq_comm_set_capacity(afq_handle *h, int max_walkers_per_peer);
int afq_comm_set_timeout(afq_handle *h, double seconds);
int afq_comm_probe(afq_handle *h, int64_t *mismatch_out);
int afq_comm_stats(afq_handle *h, int64_t *out);
int afq_comm_parent_ix(afq_handle *h, int32_t *parent_ix_global);
int afq_estimates_allreduce(afq_handle *h, double *buf, int nest);
int afq_comm_init_local(afq_handle **handles, int n);
int afq_popcontrol_comb_local(afq_handle **handles, int n, double r, double target_weight,
                              int32_t *parent_ix_global, double *total_weight_out);
int afq_estimates_allreduce_local(afq_handle **handles, int n);
/* multi-rank building blocks: scale weights by 1/scale saving unscaled_weight
 * (handler.py:244-246); copy walker src -> dst inside this GPU; pack / unpack
 * one walker to a device buffer of afq_walker_pack_bytes bytes for transport;
 * reset all weights to 1 (handler.py:337-338).
 * What a walker carries is listed ONCE, in csrc/walker_fields.h; the copy, the pack, the clones of the population
 * control and the exchange slots of the communicator all loop over that list.  The packed walker starts
 * phi c128[M, na + nb] | ot, hybrid energy, phase, eloc (c128) | unscaled weight, detR, weight, log detR (f64);
 * the back-propagation state and walker.G follow when they are on, every entry at a multiple of the unit it is
 * copied in (16, 8 or 4 bytes) and the whole rounded up to 16 bytes:
 * 16 (per + 4) + 32 [+ 16 (per + nbp K + 1) + 16] [+ 32 M^2] bytes, per = M (na + nb).                            */
int afq_walkers_scale_weights(afq_handle *h, double scale);
int afq_walkers_copy(afq_handle *h, int src, int dst);
int afq_walker_pack_bytes(afq_handle *h, int64_t *bytes);
int afq_walker_pack(afq_handle *h, int iw, void *dev_buf);
int afq_walker_unpack(afq_handle *h, int iw, const void *dev_buf);
int afq_walkers_reset_weights(afq_handle *h);
/* estimators/mixed.py:180-225: accumulate the 10 mixed estimators over all
 * walkers on the device; eval_energy != 0 runs afq_greens + afq_local_energy. */
int afq_estimates_update(afq_handle *h, int eval_energy);
/* Mixed estimator with one_rdm: True (estimators/mixed.py:226-233,279-283): after afq_estimates_rdm(h, 1) every
 * afq_estimates_update also adds sum_w weight_w Re(G_w) to a device accumulator f64[2, M, M], where G_w is
 * walker.G as the reference leaves it: the Green's function evaluated before the step's propagation
 * (propagation/continuous.py:245), refreshed on energy steps, cloned with the walker by the comb.
 * afq_estimates_rdm_get returns (and optionally zeroes) the accumulator.  Single determinant.  With a communicator
 * walker.G travels with a walker cloned to another rank (exchange slot, afq_walker_pack) and afq_estimates_allreduce
 * reduces the accumulator along with the ten estimators (the reference keeps them in one vector, mixed.py:261).  */
int afq_estimates_rdm(afq_handle *h, int on);
/* Mixed estimator with two_rdm: 'structure_factor' (estimators/mixed.py:103-108,230-233): after afq_estimates_sf(h, 1)
 * every afq_estimates_update that evaluates the energy also adds sum_w weight_w Re two_rdm[G_w] (afq_ueg_pair_sums on
 * the walkers' mixed Green's functions) to a device accumulator f64[2, 2, nq]: weight_w is the factor that multiplies the
 * walker's energy in ENumer in that same update, so that accumulator / EDenom is the energy's own estimator per
 * momentum transfer.  UEG, single determinant, importance sampling (AFQ_EUNSUPPORTED otherwise).
 * afq_estimates_sf_get returns (and optionally zeroes) the accumulator.                                        */
int afq_estimates_sf(afq_handle *h, int on);
int afq_estimates_sf_get(afq_handle *h, double *sf_out /* f64[2, 2, nq] */, int zero);
int afq_estimates_rdm_get(afq_handle *h, double *rdm_out /* f64[2, M, M] */, int zero);
/* Synchronises the stream; also the place where a population that collapsed in an asynchronous comb is
 * reported (AFQ_EWEIGHT, walkers/handler.py:236-241) and an exchange overflow (AFQ_EOVERFLOW).           */
int afq_estimates_get(afq_handle *h, double *est_out /* c128[10] */, int zero);
/* The same without blocking at enqueue time: _begin enqueues the copy of the sums (and their zeroing) behind the work
 * already in the stream, _end waits for that copy only -- work enqueued after _begin keeps running.  One fetch in flight
 * at a time (AFQ_ESTATE).                                                                                            */
/* The next afq_propagate (or afq_propagate_finish) also takes the estimator terms of its step along, as an
 * afq_estimates_update(h, 0) called right behind it would have added them: the weight update adds every walker's terms
 * to per-walker accumulators, and the next afq_estimates_update, or the next fetch / all-reduce, folds those into the
 * sums.  For a step that neither combs nor evaluates the energy this saves the launch of the summation kernel.
 * The call also tells the library that nothing but the next step's force bias will read the Green's function this step
 * leaves behind: where that force bias contracts Ghalf_a + Ghalf_b (generic system, both spins sharing the half-rotated
 * Cholesky block, hybrid weights) the per-spin Ghalf is not stored; afq_local_energy / afq_walkers_get(AFQ_F_GHALF)
 * called afterwards evaluate it first (same numbers, one more kernel).
 * Continuous propagator, not with afq_estimates_rdm on.                                                            */
int afq_estimates_fuse_next(afq_handle *h);
int afq_estimates_get_begin(afq_handle *h, int zero);
/* afq_estimates_update(h, eval_energy) followed by afq_estimates_get_begin(h, zero) as ONE call: the summation launch of the
 * update writes the block's sums into the mapped host buffer itself (estimators/mixed.py:211-225 + :261-273 of the step
 * that ends a block) -- one launch less at every block boundary; afq_estimates_get_end collects them as after _get_begin. */
int afq_estimates_update_publish(afq_handle *h, int eval_energy, int zero);
int afq_estimates_get_end(afq_handle *h, double *est_out /* c128[10] */);

/* ---- finite-temperature AFQMC: thermal walkers of the Hubbard model, discrete Hirsch fields -----------------
 * qmc/thermal_afqmc.py, walkers/thermal.py, walkers/stack.py, thermal_propagation/hubbard.py of the reference:
 * ThermalDiscrete with the spin decomposition (every matrix real), OneBody trial density matrix, constrained
 * path, low_rank off.  A thermal walker has no determinant: it carries G_s = [I + B_L .. B_1]^-1 per spin
 * (AFQ_F_THERMAL_G) and a stack of nbins = ntime_slices / stack_size propagator products (AFQ_F_THERMAL_STACK); the
 * time slice, block and in-bin counter are the same for every walker and belong to the handle.  No trial determinant
 * and no afq_set_propagator are needed.  M <= 64 sites (a walker's working set stays in LDS).
 *   afq_thermal_configure  after afq_set_system_hubbard and afq_walkers_alloc.  BT, BT_inv (the trial's dmat and its
 *                          inverse), BH1 = expm(-dt (H1 - mu I)): f64[2, M, M]; auxf f64[2, 2] = [field][spin] with the
 *                          chemical-potential shift folded in; nstblz the period of the stable rebuild of G;
 *                          stack_size must divide ntime_slices.  options: AFQ_THERMAL_* bits of what the caller
 *                          was asked for -- each of them is refused by name.  Ends with afq_thermal_reset.
 *                          AFQ_EUNSUPPORTED: the option bits, M > 64 (M > 128 with AFQ_THERMAL_DELAYED), a system that is not Hubbard, a communicator
 *                          of more than one rank, a handle with back-propagation, ITCF or the mixed RDM switched on
 *                          (and afq_bp_configure, afq_itcf_configure, afq_estimates_rdm, afq_popcontrol_pair_branch
 *                          on a thermal handle afterwards).
 *   afq_thermal_reset      handler.py:424-430: every bin = BT^stack_size, G = the trial's stratified G (computed once,
 *                          broadcast), weight = 1, counters zeroed.
 *   afq_thermal_propagate  one time slice of every walker (thermal_propagation/hubbard.py:117-142): for the sites in
 *                          order probs = 1/2 prod_s (1 + (1 - G_s[i,i]) (auxf[x,s] - 1)), p = max(probs, 0),
 *                          norm = p_0 + p_1; u[w, i] is consumed whatever norm is; norm > 0: weight *= norm exp(eshift),
 *                          x = u < p_0 / norm ? 0 : 1, rank-1 update of both G_s; else weight = 0 and G is left alone.
 *                          Then B_s = diag(auxf[x, s]) BH1_s goes onto the current bin (stack.py:287-297), every
 *                          nstblz slices G is rebuilt from the stack (afq_thermal_greens at the slice just done), and
 *                          before the last slice G_s <- BT_s G_s BT_s^-1.  u f64[nw, M]; fields_out int32[nw, M] (may
 *                          be NULL; -1 where norm <= 0).  AFQ_ESTATE once ntime_slices slices are done.
 *   afq_thermal_greens     walkers/thermal.py:472-543 for every walker at slice_ix: the stratified decomposition of
 *                          the chain of bins starting behind bin slice_ix / stack_size, graded by column-pivoted
 *                          Householder QR (k_thermal.hip).
 *   afq_thermal_energy     P_s = I - G_s^T into the full-G Hubbard energy: E_out f64[nw, 3] = (E, T, V),
 *                          nav_out f64[nw] = tr P_up + tr P_down (either may be NULL).
 *   afq_thermal_state      int32[4] = time slice, block, in-bin counter, nbins.
 * afq_popcontrol_comb on a thermal handle copies G and the bins of parent to child (single rank);
 * afq_cap_weights, afq_walkers_get / _set of WEIGHT and UNSCALED_WEIGHT work as for ground-state walkers.         */
#define AFQ_THERMAL_CHARGE          1   /* charge_decomposition                */
#define AFQ_THERMAL_FREE_PROJECTION 2
#define AFQ_THERMAL_LOW_RANK        4
#define AFQ_THERMAL_AVERAGE_GF      8
#define AFQ_THERMAL_STREAMED_GREENS 16  /* honoured by afq_thermal_configure_continuous (below), refused here by name */
#define AFQ_THERMAL_WIDE            32  /* honoured by the two continuous entry points (below), refused here by name */
#define AFQ_THERMAL_DELAYED         128 /* honoured by afq_thermal_configure alone: the delayed-update route (below);
                                           AFQ_EINVAL on the two continuous entry points, by name */
#define AFQ_THERMAL_FAR             256 /* honoured by the two continuous entry points (below), refused here by name
                                           (64 stays an unknown bit on every entry point) */
#define AFQ_THERMAL_QUAD 512            /* honoured by the two continuous entry points (below), refused here by name */
int afq_thermal_configure(afq_handle *h, int ntime_slices, int stack_size, int nstblz, const double *BT,
                          const double *BT_inv, const double *BH1, const double *auxf, int options);
/* With AFQ_THERMAL_DELAYED in options the handle takes the real walkers' second route, for any M >= 1: every Green's
 * function (afq_thermal_reset, _greens, the rebuild of _propagate) is made by thermal_greens_wide_kernel -- the wide
 * engine of the continuous fields on real matrices: one matrix of 8 M (M | 1) bytes in LDS, two columns per lane, four
 * [M, M] buffers of device memory per (walker, spin) -- and the slice by thermal_slice_delayed_kernel: the M single-site
 * updates as delayed (blocked) updates, G in device memory, per panel of 16 sites the panel's columns and rows current
 * in LDS and G <- G + U W as one fp64 MFMA product.  The fields are those of the direct route wherever no decision lies
 * within rounding of its threshold; G, the stack and the weights agree to rounding, not to the bit.  The bound is the
 * smallest of the kernels' LDS (8 (M (M | 1) + 1152) + 512 bytes for the Green's function, 141,824 at M = 128) and the
 * 128 columns of two per lane: M <= 128 = afq_thermal_delayed_max_basis(); above it AFQ_EUNSUPPORTED with M and the
 * numbers, before stack_size is looked at.  Bits 16 and 32 next to it are refused as without it.
 * afq_thermal_estimates with AFQ_THERMAL_EST_AVERAGE_GF on such a handle is AFQ_EUNSUPPORTED (no sweep kernel).  Without
 * the bit nothing changes: M > 64 is refused. */
int afq_thermal_reset(afq_handle *h);
/* the largest M a handle configured with AFQ_THERMAL_DELAYED admits (no handle, no device) */
int afq_thermal_delayed_max_basis(void);
/* the number of device blocks the handle has allocated since afq_create (every buffer of the handle goes through one
 * allocator): a thermal handle's buffers, the wide Green's function's scratch included, are allocated by its configure
 * call, so the count stands still over afq_thermal_propagate / _greens / _reset.  AFQ_EINVAL: a NULL argument. */
int afq_thermal_device_allocations(afq_handle *h, int64_t *out);
int afq_thermal_propagate(afq_handle *h, const double *u, int32_t *fields_out, double eshift);
int afq_thermal_greens(afq_handle *h, int slice_ix);
int afq_thermal_energy(afq_handle *h, double *E_out, double *nav_out);
int afq_thermal_state(afq_handle *h, int32_t *out4);

/* ---- the mixed estimator's sums of a thermal population (estimators/mixed.py:180-233 of the reference), every kind of
 * thermal handle.  Without AVERAGE_GF: G rebuilt at the handle's current slice and its energies, bit for bit what
 * afq_thermal_greens(h, slice) + afq_thermal_energy give; cols_out f64[nw, 4] = (E, T, V, nav) per walker, per_bin_out
 * (or NULL) gets the same as its one row.  With AVERAGE_GF: for ts = 0 .. nbins - 1 the Green's function at
 * slice_ix = ts stack_size and its (E, T, V, nav) -- per_bin_out f64[nbins, nw, 4] in that order, each bit for bit the
 * loop's -- and cols_out their SUMS, added in ts order from zero (the caller multiplies by the weight and divides by
 * nbins, mixed.py:195-199).  The whole sweep is one launch per stage (Green's functions on a grid (2 nw, bins), P, energy,
 * sums) whatever nbins is, taken in chunks of whole bins when its scratch (G, P, and the engine's own scratch for every
 * work-group: per bin 2 M M nw (sizeof G + 16) bytes, + 64 M M nw streamed, + 32 nw (4 M M + M (M | 1)) far) exceeds the budget: 2 GiB unless
 * afq_thermal_set_sweep_budget says otherwise (0: the default; a chunk holds at least one bin; chunking changes no bit).
 * Afterwards the walkers' G (and det, complex kinds) are what afq_thermal_greens(h, (nbins - 1) stack_size) leaves.
 * ONE_RDM: one_rdm_out f64[2, M, M] = sum_w weight_w Re G_w of the G the call leaves, every walker in walker order.
 * TWO_RDM (UEG): two_rdm_out f64[2, 2, nq] = sum_w weight_w Re two_rdm[P_w] of the same G, from the pair sums of the
 * energy launch.  AFQ_ESTATE: no thermal configuration; AFQ_EINVAL: unknown bits in what, a needed output NULL;
 * AFQ_EUNSUPPORTED: TWO_RDM on a Hubbard handle; AVERAGE_GF on a handle configured with AFQ_THERMAL_WIDE or
 * AFQ_THERMAL_DELAYED (a handle configured with AFQ_THERMAL_FAR or AFQ_THERMAL_QUAD runs it). */
#define AFQ_THERMAL_EST_AVERAGE_GF 1
#define AFQ_THERMAL_EST_ONE_RDM    2
#define AFQ_THERMAL_EST_TWO_RDM    4   /* UEG walkers only: AFQ_EUNSUPPORTED otherwise */
int afq_thermal_estimates(afq_handle *h, int what, double *cols_out, double *per_bin_out, double *one_rdm_out,
                          double *two_rdm_out);
int afq_thermal_set_sweep_budget(afq_handle *h, size_t bytes);

/* ---- finite-temperature AFQMC with continuous fields: thermal walkers of the uniform electron gas -----------
 * thermal_propagation/planewave.py:219-276,445-517, walkers/stack.py:299-324, walkers/thermal.py of the reference:
 * PlaneWave with the phaseless constraint and the force bias, OneBody trial density matrix (diagonal for plane
 * waves), full-rank walkers.  The walker's matrices are complex: AFQ_F_THERMAL_G c128[2, M, M], AFQ_F_THERMAL_STACK
 * c128[nbins, 2, M, M], AFQ_F_THERMAL_RIGHT, AFQ_F_THERMAL_M0; the comb, afq_walkers_copy and the pack carry all four.
 * M <= 47 plane waves: the complex Green's function keeps 4 matrices of 16 M (M | 1) bytes in the 160 KiB of LDS of
 * a work-group (the shells 7, 19, 27, 33 fit, 57 does not).  With AFQ_THERMAL_STREAMED_GREENS in options every
 * Green's function of the handle (afq_thermal_greens, _propagate_continuous, _reset) is made by the streamed form of
 * the same engine: 2 matrices in LDS, T in nw * 2 * 2 * M^2 * 16 bytes of device memory of the handle's, the same
 * bits.  The bound is then the smallest of the slice kernel's 48 M (M | 1) bytes of LDS, the streamed kernel's LDS and
 * the 64 lanes of a wave: M <= 57, the next shell.  The bit is honoured, not refused; above the bound the call is
 * refused with M, the kernel that does not fit, its bytes and the bound.  Without the bit nothing changes.
 * With AFQ_THERMAL_WIDE the handle takes a third route instead (the two bits together are AFQ_EINVAL): the Green's
 * function (thermal_cgreens_wide_kernel) and the slice kernel (thermal_cslice_wide_kernel, Hubbard:
 * thermal_cslice_dense_wide_kernel) keep ONE complex matrix of 16 M (M | 1) bytes in LDS, a lane owns two columns, and
 * everything else lives in nw * 2 * 4 * M^2 * 16 bytes of device memory of the handle's.  The bound is the Green's
 * kernel's 16 (M (M | 1) + 1152) + 512 bytes of LDS: M <= 95 = afq_thermal_wide_max_basis(), which holds the shells of
 * 81 and 93 plane waves (138,384 + 18,944 bytes at M = 93) and the 8 x 8 and 9 x 9 Hubbard lattices.  The same
 * algorithm, carried differently (reflectors applied in place of an accumulated Q, LU and substitution in place of
 * Gauss-Jordan): G and det G agree with the other two routes to rounding, not to the bit; the slice kernels' right and
 * bins are the same bits.  afq_thermal_reset / _greens / _energy / _state, the comb, afq_walkers_copy and the pack
 * serve a wide handle; afq_thermal_estimates runs ONE_RDM and TWO_RDM on it and refuses AVERAGE_GF by name
 * (AFQ_EUNSUPPORTED: the wide route has no sweep kernel yet).
 * With AFQ_THERMAL_FAR the handle takes a fourth route (the bit beside AFQ_THERMAL_WIDE or AFQ_THERMAL_STREAMED_GREENS
 * is AFQ_EINVAL): the wide route with no matrix in LDS.  The Green's function (thermal_cgreens_far_kernel) is the wide
 * body with its one matrix as a fifth buffer of pitch M | 1 behind the four [M, M] of the work-group's scratch --
 * nw * 2 * (4 M^2 + M (M | 1)) * 16 bytes of device memory of the handle's, allocated by the configure call -- and the
 * vectors alone in LDS (18,944 bytes); the slice kernels (thermal_cslice_far_kernel, Hubbard:
 * thermal_cslice_dense_far_kernel) read every operand where it lies in device memory.  The same arithmetic behind other
 * loaders: G, det G, right, the bins, M0 and the weights are the bits of the wide route wherever both run.  The bound
 * is the 128 columns of two per lane: M <= 128 = afq_thermal_far_max_basis(), which holds the shell of 123 plane waves
 * and the 10 x 10, 11 x 11 and 8 x 16 Hubbard lattices; above it AFQ_EUNSUPPORTED with M and the numbers.  A far handle
 * is served as a wide one is, and afq_thermal_estimates runs AVERAGE_GF on it as well: the sweep is the same kernel on a
 * grid (2 nw, bins) (thermal_cgreens_far_sweep_kernel), every work-group in a scratch of its own.
 * With AFQ_THERMAL_QUAD the handle takes a fifth route (the bit beside AFQ_THERMAL_FAR, AFQ_THERMAL_WIDE or
 * AFQ_THERMAL_STREAMED_GREENS is AFQ_EINVAL): the far route with four columns per lane.  The Green's function
 * (thermal_cgreens_quad_kernel) is the far body with a lane owning the columns c, c + 64, c + 128 and c + 192 and its
 * vectors in LDS at 256 entries (37,888 bytes); the scratch is the far route's, nw * 2 * (4 M^2 + M (M | 1)) * 16
 * bytes (2.7 GB at M = 256 and 256 walkers), allocated by the configure call; the slice kernels
 * (thermal_cslice_quad_kernel, Hubbard: thermal_cslice_dense_quad_kernel) are the far ones with bv at 256 entries.
 * Every column goes through the far route's operations in the far route's order: G, det G, right, the bins, M0 and the
 * weights are the bits of the far route wherever both run.  The bound is the 256 columns of four per lane:
 * M <= 256 = afq_thermal_quad_max_basis(), which holds the shells of 147 to 251 plane waves and the 12 x 12 and
 * 16 x 16 Hubbard lattices; above it AFQ_EUNSUPPORTED with M and the numbers.  A quad handle is served as a far one is,
 * AVERAGE_GF included (thermal_cgreens_quad_sweep_kernel).
 *   afq_thermal_configure_continuous  after afq_set_system_ueg (index lists over ALL plane waves, for the energy) and
 *                          afq_walkers_alloc; no trial determinant, no afq_set_propagator.  BT, BT_inv, BH1
 *                          f64[2, M, M]: the trial's dmat and its inverse (diagonal) and
 *                          expm(-dt/2 h1e_mod + dt/2 mu) of which the diagonal is read, as the reference reads it;
 *                          mf_shift c128[K]; dt becomes the handle's time step; a component of the force bias with
 *                          |xbar| > fb_bound (the reference's default: 1.0) is scaled to unit modulus (counted in
 *                          afq_counters [0]).  The exponential is the degree-6 polynomial.  options:
 *                          AFQ_THERMAL_* bits of what the caller was asked for, refused by name.  Ends with
 *                          afq_thermal_reset.  AFQ_EUNSUPPORTED: the option bits, a system that is not the UEG,
 *                          M > 47 (the message carries M and the bytes; M > 57 with
 *                          AFQ_THERMAL_STREAMED_GREENS, M > 95 with AFQ_THERMAL_WIDE, M > 128 with
 *                          AFQ_THERMAL_FAR, M > 256 with AFQ_THERMAL_QUAD), a trial that is not diagonal, more than
 *                          one rank, back-propagation / ITCF / mixed RDM on the handle.
 *   afq_thermal_propagate_continuous  one time slice of every walker, dead ones included: P = I - G^T,
 *                          xbar = -sqrt(dt) P.[iA | iB] (|xbar_i| > fb_bound: unit modulus), xs = xi - xbar, cmf = -sqrt(dt) xs.mf_shift,
 *                          cfb = xi.xbar - xbar.xbar / 2, VHS = sqrt(dt) (iA xs[:nq] + iB xs[nq:]),
 *                          B_s = diag(BH1_s) (sum_{n <= 6} VHS^n / n!) diag(BH1_s); right_s <- B_s right_s (right = I
 *                          at the first slice of a bin), bin[block]_s = left_k right_s with
 *                          left_k = BT^stack_size BT_inv^k after the k-th slice of the bin;
 *                          G_s = [I + bin[nbins - 1] .. bin[0]]^-1, Mnew_s = det G_s;
 *                          oratio = M0_up M0_dn / (Mnew_up Mnew_dn), hyb = log(oratio) + cfb + cmf,
 *                          magn = |exp(hyb)|; a zero denominator or a magn that is not finite (NaN included): weight = 0, M0 kept; else
 *                          weight *= magn max(0, cos Im(hyb - cfb)) and M0 = Mnew.  xi f64[nw, K], or NULL for the
 *                          device's Philox stream; xi_out f64[nw, K] (may be NULL): the fields used.
 *   afq_thermal_reset / _greens / _energy / _state serve this kind of handle too.  reset also sets right = I; it leaves
 *   M0 alone, as the reference's Walkers.reset does (the first slice of the next path divides by the determinant the
 *   last path ended with); only afq_thermal_configure_continuous sets M0 = det of the trial's G.  greens leaves
 *   det G_s in AFQ_F_THERMAL_DET; energy is the UEG energy of P_s = I - G_s^T (real parts) and
 *   nav = Re(tr P_up + tr P_down).                                                                             */
int afq_thermal_configure_continuous(afq_handle *h, int ntime_slices, int stack_size, double dt, const double *BT,
                                     const double *BT_inv, const double *BH1, const double *mf_shift, double fb_bound,
                                     int options);
int afq_thermal_propagate_continuous(afq_handle *h, const double *xi, double *xi_out);
/* the largest M a handle configured with AFQ_THERMAL_WIDE admits (no handle, no device) */
int afq_thermal_wide_max_basis(void);
/* the largest M a handle configured with AFQ_THERMAL_FAR admits (no handle, no device) */
int afq_thermal_far_max_basis(void);
/* the largest M a handle configured with AFQ_THERMAL_QUAD admits (no handle, no device) */
int afq_thermal_quad_max_basis(void);

/* ---- finite-temperature AFQMC with continuous fields: thermal walkers of the Hubbard model --------------------
 * thermal_propagation/continuous.py:84-120,202-257 (Continuous, phaseless, force bias, hybrid weight) with
 * thermal_propagation/hubbard.py:199-250 (HubbardContinuous, the charge form) and the non-diagonal branch of
 * walkers/stack.py:299-324.  The walkers are the complex ones above; the trial's density matrix and BH1 are dense and
 * real, the field exponential is a diagonal.
 *   afq_thermal_configure_hubbard_continuous  after afq_set_system_hubbard and afq_walkers_alloc.  BT, BT_inv, BH1
 *                          f64[2, M, M], all dense: the trial's dmat, its inverse, and
 *                          expm(-dt/2 (h1e_mod - i sqrt(U) diag(mf_shift) + sign mu)); mf_shift c128[M] =
 *                          i sqrt(U) diag(P_up + P_dn) of the trial; mf_const_fac c128[1] = exp(-dt mf_shift.mf_shift / 2).
 *                          left_k = BT^stack_size BT_inv^(k + 1) is built on the host in the reference's order.
 *                          options: AFQ_THERMAL_STREAMED_GREENS, AFQ_THERMAL_WIDE, AFQ_THERMAL_FAR or AFQ_THERMAL_QUAD is honoured (two
 *                          of them: AFQ_EINVAL; with WIDE the bound is M <= 95, with FAR M <= 128, with QUAD M <= 256, as above), the other AFQ_THERMAL_* bits are
 *                          refused by name.  Without WIDE the bound on M is the smallest of the slice kernel's
 *                          40 M (M | 1) + 1024 bytes of LDS (M <= 63), the Green's kernel's (M <= 47 resident, 64
 *                          streamed) and the 64 lanes of a wave: M <= 47, and M <= 63 with the bit.  Above it
 *                          AFQ_EUNSUPPORTED names M, the kernel that does not fit, its bytes and the bound.  Also
 *                          refused: a system that is not Hubbard, more than one rank, back-propagation / ITCF /
 *                          mixed RDM on the handle.  Ends with afq_thermal_reset and M0 = det of the trial's G.
 *   afq_thermal_propagate_continuous  on such a handle: vbias_i = i sqrt(U) (P_up,ii + P_dn,ii),
 *                          xbar = -sqrt(dt) (vbias - mf_shift), |xbar_i| > 1 scaled to unit modulus (each counted in
 *                          afq_counters [0]), xs, cmf, cfb as above; BV = diag(sum_{n <= 6} v^n / n!),
 *                          v = sqrt(dt) i sqrt(U) xs; B_s = BH1_s (BV BH1_s); the stack, G_s and Mnew_s as above;
 *                          magn = |mf_const_fac exp(hyb)|, the rest of the weight update as above.  K = M fields.
 *   afq_thermal_reset / _greens / _energy / _state serve it; energy is the Hubbard energy of P_s = I - G_s^T.
 *   afq_thermal_left_table  the host-side table the configuration uploads, for inspection (no handle, no device):
 *                          BTpow_out f64[2, M, M] = BT left-multiplied stack_size times onto I and left_out
 *                          f64[stack_size, 2, M, M], left_k = left_(k - 1) BT_inv, in the reference's order of
 *                          operations (walkers/stack.py:238-243,309-310), every element one chain of fused
 *                          multiply-adds over k ascending.                                                        */
int afq_thermal_left_table(int M, int stack_size, const double *BT, const double *BT_inv, double *BTpow_out, double *left_out);
int afq_thermal_configure_hubbard_continuous(afq_handle *h, int ntime_slices, int stack_size, double dt, const double *BT,
                                             const double *BT_inv, const double *BH1, const double *mf_shift,
                                             const double *mf_const_fac, int options);

/* ---- misc ------------------------------------------------------------------ */
/* Device stream of auxiliary fields (used by afq_propagate with xi == NULL; replaces numpy.random.normal of
 * propagation/continuous.py:133 when parity with the host stream is not required): Philox4x32-10 (Salmon et
 * al., SC'11), counter = (element pair index, launch counter ^ stream hash), key = seed, Box-Muller on two
 * 53-bit uniforms.  `stream` must differ between ranks (qmc/utils.py:14 seeds seed + rank).
 *   afq_rng_normal      the next n normals of the stream (what the next afq_propagate would have used)
 *   afq_rng_philox4x32  the bare block function for known-answer tests: ctr_key uint32[n][6] =
 *                       (counter[4], key[2]) -> out uint32[n][4]                                          */
int afq_rng_seed(afq_handle *h, uint64_t seed, uint64_t stream);
int afq_rng_normal(afq_handle *h, double *out, int64_t n);
int afq_rng_philox4x32(afq_handle *h, const uint32_t *ctr_key, uint32_t *out, int n);
/* Diagnostics.  Every kernel launch leaves its name in a host-side ring of the handle; afq_last_launch formats
 * "api=<entry point> queued=<n> [retired=<m> first-unretired=<kernel>] last: <names>" into buf and may be
 * called from a watchdog thread while the owning thread is blocked in a synchronising call (host memory only).
 * afq_debug(h, sync, markers): sync != 0 synchronises and checks after every launch (a failing kernel is named
 * in afq_last_error); markers != 0 queues a one-thread marker behind every launch so that `retired` counts the
 * launches that completed.  Environment: AFQ_DEBUG_SYNC=1, AFQ_DEBUG_MARKERS=1 set them at afq_create.     */
int afq_debug(afq_handle *h, int sync_every_launch, int markers);
int afq_last_launch(afq_handle *h, char *buf, int len, uint64_t *queued, uint64_t *retired);
/* Guard bands and poison on the handle's device memory, a debugging mode selected by the environment at afq_create:
 * AFQ_DEBUG_GUARD=1 puts a band of AFQ_DEBUG_GUARD_BYTES (a multiple of 4096; 4096 by default) in front of and behind every
 * device block of the handle -- its owned blocks, its per-call buffers and the plane-wave tables -- filled with a 32-bit word
 * that reads as NaN as a float and as a double; AFQ_DEBUG_GUARD=2 also fills the block itself before it is handed out, with
 * a second NaN word where its elements are double, complex or float and with zeros elsewhere (an index is never poisoned).
 * Both bands of a block are compared with the pattern, after a device synchronisation, before the block is freed.  The
 * communicator's windows and exchange buffers (afq_comm_*) stay out of the mode: peers address them.  Unset or 0: nothing of
 * this happens.
 *   afq_debug_guard_check   the same comparison for every live block of the handle, without freeing (which call broke a band)
 *   afq_debug_guard_report  the number of violations logged by this process so far; their text, one per line ("<block>:
 *                           <front|back> band, first differing byte at offset <o> of a block of <n> bytes, word 0x...", o
 *                           relative to the block: -1 is the byte in front of it, n the first behind it), goes to buf[n]
 *   afq_debug_guard_reset   clears that log                                                                        */
int afq_debug_guard_check(afq_handle *h);
int afq_debug_guard_report(char *buf, int n);
void afq_debug_guard_reset(void);
/* counters: [0]=nfb_trig (continuous.py:150), [1]=nhe_trig (:210,213), [2]=overlap matrices the blocked
 * Gauss-Jordan flagged as poorly conditioned block-wise and handed to the step-by-step kernel (diagnostic),
 * [3]=walker steps the fused propagator took through its closed-shell deal (spin blocks bitwise equal)       */
int afq_counters(afq_handle *h, int64_t *out, int reset);
/* the same, first n counters (n <= 10; [8]=walker steps whose overlap matrix was made and inverted under the fused propagator's
 * closing pass, afq_set_step_tail_overlap; [9]=walker steps that started from the step hand-over, afq_set_step_handover): [4]=walker energy evaluations whose exchange energy was evaluated for one spin and
 * counted twice (closed-shell population, decided on the device: energy_finish_kernel), [5]=walker Green's functions
 * computed for one spin (closed-shell walker, greens_small_kernel), [6]=per-determinant overlaps of a multi-determinant
 * trial that came out as NaN (0 x inf behind a zero pivot of a singular overlap matrix) and were taken as zero overlaps,
 * [7]=walker steps that went through the large-system GEMM chain (M > 128) as closed-shell walkers: alpha columns only in the
 * one-body and Taylor products, copied over the beta block behind the chain (closed_flags_kernel)                      */
int afq_counters_ext(afq_handle *h, int64_t *out, int n, int reset);
/* accumulated device ms per phase: [0] greens [1] one-body [2] force bias+fields
 * [3] vhs [4] exponential [5] overlap+weight [6] reortho [7] energy            */
int afq_timers(afq_handle *h, double *out_ms, int reset);
int afq_enable_timers(afq_handle *h, int on);
/* HIP stream of the handle (hipStream_t as void*) */
int afq_stream(afq_handle *h, void **stream);
/* Per-launch durations of the hot kernels, HIP events recorded on the handle's
 * stream around the launch (no host synchronisation until _get): bench.py's
 * live roofline measurement over its timed region.  afq_kernel_trace(h, 1)
 * clears and starts recording every kind (up to 4096 launches per kind),
 * (h, 2 << kind | ...) only the selected kinds (an event pair costs a few
 * microseconds of pipeline bubble per launch), (h, 0) stops.
 * afq_kernel_trace_stride(h, kind, n): only every n-th launch of that kind is timed (n >= 1, default 1), so that
 * sampling inside a timed region costs 1 / n of those bubbles.                                                  */
#define AFQ_K_PROPAGATOR 0   /* fused B exp(V) B kernel (k_fused.hip)          */
#define AFQ_K_EXCHANGE 1     /* Cholesky exchange-energy kernel (k_energy.hip) */
#define AFQ_K_VHS 2          /* HS potential GEMM                              */
#define AFQ_K_FORCE_BIAS 3   /* force-bias GEMM                                */
#define AFQ_K_GREENS 4       /* Green's function kernel (N <= 45 path)         */
#define AFQ_K_COUNT 5
int afq_kernel_trace(afq_handle *h, int on);
int afq_kernel_trace_stride(afq_handle *h, int kind, int stride);
int afq_kernel_trace_get(afq_handle *h, int kind, double *ms_out, int max_n, int *n_out);
/* Profile pass over EVERY launch of the library, whatever the configuration dispatches to: afq_launch_trace(h, 1)
 * clears and starts recording an event pair around each launch (up to 65536), keyed by the name the launch leaves in
 * the breadcrumb ring (the kernel for plain launches, the launching function for the GEMM engines: k_onebody,
 * k_vhs_generic ...); (h, 0) stops.  afq_launch_trace_get synchronises and returns, per distinct name, the summed
 * duration and the number of launches: names_out receives the names back to back, NUL-terminated.  The pairs cost a few
 * microseconds of bubble per launch: for an extra pass behind a timed region, not for the region itself.
 * (measurement hook, no reference counterpart)                                                                   */
int afq_launch_trace(afq_handle *h, int on);
int afq_launch_trace_get(afq_handle *h, char *names_out, int names_len, double *total_ms, int64_t *launches,
                         int max_names, int *n_out);
/* Flops the matrix pipe executed in the LAST launch of a kind: MFMA instructions x their flop count (2048 per
 * v_mfma_f64_16x16x4, 512 per 4x4x4), tile and contraction padding included, a 3-multiplication complex product
 * counted as 3.  issued / time / peak is the utilisation of the pipe; the algorithmic count of SURVEY 8d
 * (4 multiplications, no padding) over the same time is the figure comparable across implementations.
 * 0 for kinds that have not been launched or do not run on the matrix pipe.  (measurement hook, no reference
 * counterpart)                                                                                                    */
int afq_kernel_issued_flops(afq_handle *h, int kind, double *flops_out);
/* fused propagator (AFQ_K_PROPAGATOR): matrix-pipe flops ONE walker issues in the last launch's shape through the open-shell
 * deal and through the closed-shell deal (alpha slots only); afq_kernel_issued_flops reports nw x the open-shell count, the
 * count of a launch is (nw_live - n_closed) x open + n_closed x closed with n_closed from afq_counters [3]            */
int afq_propagator_issued_flops(afq_handle *h, double *open_per_walker, double *closed_per_walker);

#ifdef __cplusplus
}
#endif
#endif /* AFQMC_HIP_H */
