// Internal declarations shared by the translation units of libafqmc_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../include/afqmc_hip.h"
#include "greens_cache.h"
#include "step_state.h"
#include "dev_mem.h"

typedef double2 cplx;   // (x = re, y = im), same bytes as numpy complex128
template <> struct DevFloating<cplx> : std::true_type {};      // (dev_guard.h: a block of cplx is poisoned like one of double)

__host__ __device__ inline cplx cmake(double r, double i) { return make_double2(r, i); }
__host__ __device__ inline cplx cadd(cplx a, cplx b) { return cmake(a.x + b.x, a.y + b.y); }
__host__ __device__ inline cplx csub(cplx a, cplx b) { return cmake(a.x - b.x, a.y - b.y); }
__host__ __device__ inline cplx cmul(cplx a, cplx b) {
    return cmake(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__host__ __device__ inline cplx cconj(cplx a) { return cmake(a.x, -a.y); }
__host__ __device__ inline cplx cscale(cplx a, double s) { return cmake(a.x * s, a.y * s); }
// a += b*c
__host__ __device__ inline void cfma(cplx &a, cplx b, cplx c) {
    a.x = fma(b.x, c.x, a.x); a.x = fma(-b.y, c.y, a.x);
    a.y = fma(b.x, c.y, a.y); a.y = fma(b.y, c.x, a.y);
}
__host__ __device__ inline double cabs2(cplx a) { return a.x * a.x + a.y * a.y; }
__device__ inline cplx cdiv(cplx a, cplx b) {
    // Smith's algorithm (what C99/numpy use) to avoid overflow
    if (fabs(b.x) >= fabs(b.y)) {
        double r = b.y / b.x, d = b.x + b.y * r;
        return cmake((a.x + a.y * r) / d, (a.y - a.x * r) / d);
    } else {
        double r = b.x / b.y, d = b.x * r + b.y;
        return cmake((a.x * r + a.y) / d, (a.y * r - a.x) / d);
    }
}

#define AFQ_NSCAL 12
enum { AFQ_HS_HERMITIAN = 1, AFQ_HS_GENERAL = 2 };       // afq_handle::hs_cplx
enum { T_GREENS = 0, T_ONEBODY, T_FB, T_VHS, T_EXP, T_OVLP, T_QR, T_ENERGY, T_COUNT };

#define AFQ_NCOUNTERS 10    // afq_counters_ext (include/afqmc_hip.h)

// The kind of thermal walker a handle holds: none, real (afq_thermal_configure), complex with a diagonal trial
// (afq_thermal_configure_continuous), complex with a dense trial (afq_thermal_configure_hubbard_continuous)
enum ThKind { TH_NONE = 0, TH_REAL, TH_CPLX_DIAG, TH_CPLX_DENSE };
// Where a thermal handle's Green's function (and, WIDE, its slice kernel) keeps its matrices: the route chosen by the
// option bits of the configure call.  RESIDENT: all in LDS.  STREAMED (AFQ_THERMAL_STREAMED_GREENS, complex walkers): T in
// device memory.  WIDE (AFQ_THERMAL_WIDE, complex; AFQ_THERMAL_DELAYED, real): one matrix in LDS, two columns per lane.
// FAR (AFQ_THERMAL_FAR, complex): the wide route with that matrix in device memory as well, M <= 128.
// QUAD (AFQ_THERMAL_QUAD, complex): the far route with four columns per lane, M <= 256.
enum ThEngine { TH_ENGINE_RESIDENT = 0, TH_ENGINE_STREAMED, TH_ENGINE_WIDE, TH_ENGINE_FAR, TH_ENGINE_QUAD };

struct afq_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    DevMem mem;                     // the owning slots of every device block below, by lifetime (dev_mem.h)

    // ---- system
    int kind = 0;
    int M = 0, K = 0, na = 0, nb = 0, nt = 0;
    double ecore = 0.0;
    // generic
    double *hs_pot = nullptr;       // f64, TRANSPOSED: [K, ld_hs] with ld_hs = M*M rounded up to even (zero pad)
    bool hs_sym = false;            // L_n symmetric: hs_pot holds only the columns (p <= q), [K, ld_hs]
    double *L_full = nullptr;       // [K, M, Mp] every L_n as a padded row-major matrix (full-G energy; built on first use)
    int2 *hs_pair = nullptr;        // [M(M+1)/2] (p, q) of every packed column
    // complex Cholesky vectors (afq_set_system_generic_c128): hs_pot holds Re L and hs_pot_im Im L, both transposed.
    // Hermitian L (L_n[q,p] == conj(L_n[p,q])): Re L packed p <= q as in the symmetric real case (hs_pair), Im L
    // packed p < q (hs_pair_im); general L: both panels with all M*M columns.  hs_sym stays false.
    int hs_cplx = 0;                // 0 real, AFQ_HS_HERMITIAN, AFQ_HS_GENERAL
    double *hs_pot_im = nullptr;    // [K, ld_hs_im]
    int2 *hs_pair_im = nullptr;     // [M(M-1)/2] (p, q), p < q, of every packed Im column (Hermitian)
    long ld_hs_im = 0;
    cplx *L_full_c = nullptr;       // [K, M, Mp] complex L_n for the full-G energy (complex vectors only)
    long ld_hs = 0, ld_rc = 0;      // leading dimensions of hs_pot^T and of rchol_re/im (K rounded up to even)
    bool rchol_real = true;
    double *rchol_re = nullptr;     // f64 [nt*M, ld_rc]
    double *rchol_im = nullptr;     // f64 [nt*M, ld_rc] or null when real
    double *rchol_frag[2] = {nullptr, nullptr};   // energy-kernel A operand, fragment order, per spin
    double *rchol_frag_im[2] = {nullptr, nullptr};
    // quadratic-form exchange (k_energy.hip): Atil_s [(N_s M), ldq] f64 (c128 when rchol is complex), built on first use
    void *atil[2] = {nullptr, nullptr};
    bool atil_unavailable = false;  // automatic mode: Atil did not fit when it was to be built -> T-intermediate kernel
    bool rchol_same = false;        // alpha and beta blocks of rchol are bitwise equal
    int exx_mode = 0;               // afq_set_exchange_algorithm: 0 auto, 1 T-intermediate (exx_kernel), 2 quadratic form
    cplx *exq_y = nullptr;          // [2 * slices, nw, ceil(N M / 16)] per-tile partial sums of the quadratic form
    size_t exq_y_len = 0;
    cplx *H1 = nullptr;             // [2, M, M]
    cplx *rH1 = nullptr;            // half-rotated H1: [nt, M]; rH1[i][q] = sum_p conj(psi[p,i]) H1_s[p,q]
    // hubbard
    double U = 0.0;
    // ueg
    int nq = 0;
    int64_t nnzA = 0, nnzB = 0;
    int64_t *iA_colptr = nullptr, *iA_row = nullptr; cplx *iA_val = nullptr;
    int64_t *iB_colptr = nullptr, *iB_row = nullptr; cplx *iB_val = nullptr;
    // row-major (CSR over M*M rows) copies for the VHS gather
    int64_t *iA_rowptr = nullptr, *iA_col = nullptr; cplx *iA_rval = nullptr;
    int64_t *iB_rowptr = nullptr, *iB_col = nullptr; cplx *iB_rval = nullptr;
    // column-ELL copy of [iA | iB] for the LDS force-bias kernel: k-th non-zero of column c at [k * 2nq + c]
    int ell_len = 0; int *ell_row = nullptr; cplx *ell_val = nullptr;
    // rows of G the UEG energy gathers touch (the occupied orbitals of the trial): compact index per row or -1
    int ueg_nrows = 0; int *ueg_rmap = nullptr; int *ueg_rows = nullptr;
    // the energy's index lists packed for the thread-per-q kernel: (row of the staged G << 16) | column, int32 offsets
    int *ueg_kp = nullptr, *ueg_pm = nullptr, *ueg_koff = nullptr, *ueg_poff = nullptr;
    int64_t *kpq_off = nullptr, *kpq_i = nullptr, *kpq_kpq = nullptr;
    int64_t *pmq_off = nullptr, *pmq_i = nullptr, *pmq_pmq = nullptr;
    double *vqvec = nullptr; double vol = 1.0; double *H1diag = nullptr;
    void *ueg_fast = nullptr;       // k_ueg.hip: tables of the plane-wave step that needs no M x M intermediate
    // pair sums on general Green's functions (k_ueg_sf.hip): the lists packed with the rows of G itself (ueg_kp / ueg_pm
    // carry rows of the staged copy), the momentum transfers by decreasing nk * np (the first sf_nlong: a wave each)
    int *sf_kp = nullptr, *sf_pm = nullptr, *sf_order = nullptr;
    int sf_nlong = 0;
    cplx *sf_ws = nullptr, *sf_two = nullptr;      // [n, 2, nq, 3] Gkpq, Gpmq, Gprod; [n, 2, 2, nq] two_rdm; grown on demand
    size_t sf_ws_len = 0, sf_two_len = 0;
    // correlation functions (k_corr.hip): [n, 2, M] diagonals, then [nchunk, 5, M, M] partial sums; grown on demand
    cplx *corr_ws = nullptr;
    size_t corr_ws_len = 0;
    // pairing correlations (afq_set_pairing_bonds, k_pair.hip): the bond table [pair_nb, M] (partner sites, -1 = none) and
    // the partial sums [nchunk, nb, nb, M, M] of more than one chunk, grown on demand
    int *pair_nbr = nullptr;
    int pair_nb = 0;
    cplx *pair_ws = nullptr;
    size_t pair_ws_len = 0;

    // ---- trial
    bool have_trial = false;
    cplx *psi = nullptr;            // [M, nt]
    cplx *psic = nullptr;           // conj(psi) [M, nt] (B operand of the overlap GEMM)
    cplx *psicT = nullptr;          // conj(psi)^T [nt, M]: coalesced reads of the Hubbard force bias (single-determinant upload only)
    long psi_stride = 0;            // elements between per-walker 'trials' (back-propagation only; 0 = shared psi)
    bool psi_real = false;          // every imaginary part of the uploaded trial is exactly zero
    bool psi_closed = false;        // na == nb and the alpha and beta blocks of the (single, shared) trial are bitwise equal
    // Closed-shell populations (round 5).  The Green's function kernel checks every walker's spin blocks for bitwise equality
    // (greens_small_kernel); a walker that fails raises closed_bad to the epoch of that launch (gf.closed says which Ghalf
    // the verdict is about).  The host never reads the flag.
    unsigned long long *closed_bad = nullptr;
    unsigned long long closed_epoch = 0;
    // host-side HINT read with every block's sums (est_publish_kernel): the population held an open-shell walker at the last
    // block end.  launch_exx_quadratic then skips the one-spin-first form (two launches when the population is open: 181
    // against 135 us at C3) for the one-launch two-spin form; results are the same either way, a stale hint costs time only
    unsigned long long closed_epoch_pub = 0;
    bool exx_open_hint = false;
    // Large-system propagation (the GEMM chain of k_onebody / k_apply_exponential: M > 128), round 6: closed_w[w] = 1 when walker
    // w's spin blocks are bitwise equal (closed_flags_kernel, every step, on the walkers themselves: no state to keep valid).
    // While closed_large is set the one-body and Taylor GEMMs leave out the work-group tiles that lie wholly in the beta columns
    // of such a walker; closed_copy_beta_kernel copies the propagated alpha block over the beta block at the end of the step.
    int *closed_w = nullptr;
    size_t closed_w_n = 0;
    bool closed_large = false;

    // the trial-dependent operands of every determinant (multi-determinant trial: SURVEY 8a row 15), owned here;
    // psi / psic / rchol_* / rchol_frag* / atil / rH1 above and ghalf / vbias below are VIEWS of the selected one
    struct DetOps {
        cplx *psi = nullptr, *psic = nullptr, *rH1 = nullptr;
        double *rchol_re = nullptr, *rchol_im = nullptr;
        double *rchol_frag[2] = {nullptr, nullptr}, *rchol_frag_im[2] = {nullptr, nullptr};
        void *atil[2] = {nullptr, nullptr};
        bool rchol_same = false;
        GreensCache::Stamp vbias_stamp;         // this determinant's force-bias partials (as gf.vbias for one determinant)
    };
    int ndet = 1, cur_det = 0;
    std::vector<DetOps> dets = std::vector<DetOps>(1);   // size ndet
    cplx *coeffs = nullptr;         // [ndet] device copy of the CI coefficients
    cplx *detd = nullptr;           // [ndet, nw] per-determinant overlaps <D_d|phi_w>
    cplx *detd_a = nullptr;         // [ndet, nw] their alpha factors det(phi_a^T conj(D_d,a)) (multi_det.py:209 tests it first)
    cplx *detw = nullptr;           // [nw, ndet] weights conj(c_d) <D_d|phi_w> of the last evaluation
    cplx *ghalf_all = nullptr;      // [ndet] slices: what ghalf / vbias point into
    cplx *vbias_all = nullptr;
    cplx *energy_all = nullptr;     // [ndet, nw, 3] per-determinant local energies
    // force bias of a multi-determinant trial through the determinant-averaged Green's function (the reference's own
    // formulation, propagation/generic.py:154-157 + walkers/multi_det.py:283-290; k_gemm.hip: k_force_bias_msd_gbar)
    int msd_fb_mode = 0;            // afq_set_msd_force_bias: 0 auto, 1 one contraction per determinant, 2 averaged G
    bool msd_fb_gbar = false;       // the last force_bias() left ONE already-averaged set of partials in vbias_all
    cplx *msd_psicT = nullptr;      // [ndet nt, M] conj(psi_d)^T of every determinant, stacked
    cplx *msd_gs = nullptr;         // [nw, ndet nt, M] Ghalf_d scaled by w_d / sum_d w_d
    cplx *msd_S = nullptr;          // [nw, ld_hs] (Gbar + Gbar^T) on the packed columns p <= q (the diagonal: Gbar[p,p])
    double *hs_pk = nullptr;        // [M (M + 1) / 2, ld_rc] packed hs_pot with the field index contiguous
    // Hermitian complex L (hs_cplx): the antisymmetric half of the averaged-G force bias (k_force_bias_msd_gbar)
    cplx *msd_psicT_neg = nullptr;  // [ndet nt, M] -conj(psi_d)^T
    cplx *msd_D = nullptr;          // [nw, ld_hs_im] (Gbar - Gbar^T) on the packed columns p < q
    double *hs_pk_im = nullptr;     // [M (M - 1) / 2, ld_rc] packed Im L with the field index contiguous

    // ---- back-propagation (estimators/back_propagation.py, walkers/stack.py FieldConfig)
    int nbp = 0;                    // field configurations kept per walker (0 = off)
    cplx *bp_hist = nullptr;        // [nw, nbp, K] shifted fields x - xbar of the last steps
    int *bp_n = nullptr;            // [nw] FieldConfig.step
    int *bp_flag = nullptr;         // [nw] set by the weight kernel when this step's fields are recorded
    double *bp_cos = nullptr;       // [nw] running product of the cosine factors
    cplx *bp_ph = nullptr;          // [nw] running product of I / |I|
    cplx *phi_old = nullptr;        // [nw, M, nt] walker at the start of the back-propagation window
    cplx *phi_bp = nullptr;         // [nw, M, nt] back-propagated trial (+ its conjugate behind it)
    cplx *BH1dag = nullptr;         // [2, M, M] BH1^H
    cplx *bp_xs = nullptr;          // [nw, K]
    cplx *bp_est = nullptr;         // [4 + 2 M M]
    cplx *bp_ot = nullptr;          // [nw] where a re-orthogonalisation of phi_bp leaves ot and detR while the walkers'
    double *bp_detR = nullptr;      // own are parked (single-determinant windows)
    // multi-determinant windows (afq_bp_update_msd, k_bp_msd.hip): with ndet > 1 phi_bp holds [ndet, nw, M, nt] and its
    // conjugate behind it, and bpm_ws the window's own scratch (carved by afq_bp_update_msd), bpm_ws_len complex elements
    cplx *bpm_ws = nullptr;
    size_t bpm_ws_len = 0;
    // back-propagated two-body RDM / EKT Fock matrices (afq_bp_observables, k_bp_obs.hip)
    int bpo_two = 0, bpo_ekt = 0;   // what afq_bp_update_ext may be asked for
    int bpo_sf = 0;                 // two_rdm is the UEG structure factor [2, 2, nq] (afq_bp_observables(h, 2, ...))
    int bpo_corr = 0;               // two_rdm is the correlation functions [5, M, M] (afq_bp_observables(h, 3, ...), k_corr.hip)
    int bpo_pair = 0;               // two_rdm is the pairing correlations [nb, nb, M, M] (afq_bp_pairing, k_pair.hip)
    int bpo_nL = 0;                 // EKT vectors L_x, x < nL
    cplx *bpo_h1 = nullptr;         // [M, M] h1 of the EKT
    cplx *bpo_L = nullptr;          // [nL, M, M] the caller's vectors (null: the handle's own real L_full)
    cplx *bpo_wt = nullptr;         // [nw] accumulation weights of the window
    cplx *bpo_out = nullptr;        // [M^4, 4 nq, 5 M M or nb nb M M (two_rdm) + 2 M M (fock)] results of the window
    cplx *bpo_ws = nullptr;         // scratch, grown on demand
    size_t bpo_ws_len = 0;
    int bpo_nc = 0, bpo_ncy = 0;    // afq_bp_ekt_chunks: x per chunk of the panels / of the linear term (0: automatic)
    // imaginary-time Green's function (afq_itcf_configure / afq_itcf_update, k_itcf.hip): window of nmax + neqlb steps
    // on the field history above (nbp == nmax + neqlb); 0 = off
    int it_nmax = 0, it_neqlb = 0, it_stable = 1, it_restore = 0;
    cplx *it_ws = nullptr;          // the window's scratch, grown on demand
    size_t it_ws_len = 0;

    // ---- discrete Hirsch propagator (propagation/hubbard.py:12-343)
    bool hirsch = false;
    cplx hs_delta[2][2];            // auxf - 1, [field][spin]
    cplx hs_wfac[2];                // aux_wfac
    cplx hs_auxf[2][2];             // auxf exp(-dt U / 2), [field][spin]
    cplx hs_gamma;                  // arccosh(exp(+-dt U / 2)) (complex for the charge decomposition)
    bool hs_charge = false;
    bool hs_direct = false;         // single_site_update: False -- two_body_direct (hubbard.py:222-275)
    double *hs_fbfac = nullptr;     // [nw] force-bias factor of the direct update
    cplx *hs_oinv = nullptr;        // [nw, 2, nmax, nmax] inverse overlaps O^-1 (= inv_ovlp^T of the reference)
    double *hs_u = nullptr;         // [nw, M] uniforms of the site updates
    int *hs_fields = nullptr;       // [nw, M] chosen fields (-1: not visited)
    int *hs_used = nullptr;         // [nw] uniforms consumed
    int *hs_alive0 = nullptr;       // [nw] walkers the driver propagates this step (|w| > 1e-8)

    // ---- finite-temperature walkers (k_thermal.hip; walkers/thermal.py, walkers/stack.py, thermal_propagation/hubbard.py)
    ThKind th_kind = TH_NONE;       // which configure entry point succeeded last: what kind of thermal walker the handle holds
    ThEngine th_engine = TH_ENGINE_RESIDENT;   // and by which route: set by the configure calls alone
    // the route's scratch in device memory, in scalars of the walker's kind; allocated by the configure calls alone.
    // STREAMED: [nw, 2, 2, M, M], T of the Green's kernel, two buffers per work-group; WIDE: [nw, 2, 4, M, M], four per
    // work-group, of which the wide slice kernels use the walker's first two; RESIDENT: null
    void *th_scratch = nullptr;
    int th_L = 0, th_ss = 0, th_nbins = 0, th_nstblz = 0;   // time slices, stack_size, bins, stabilisation period
    int th_slice = 0, th_block = 0, th_counter = 0;          // PropagatorStack.time_slice / block / counter (every walker's)
    double th_auxf[2][2];           // [field][spin], the chemical-potential shift folded in
    double *th_BT = nullptr, *th_BTinv = nullptr, *th_BH1 = nullptr;   // [2, M, M] each
    double *th_BTpow = nullptr;     // [2, M, M] BT^stack_size: every bin of a fresh path
    double *th_G = nullptr;         // [nw, 2, M, M]
    double *th_G0 = nullptr;        // [2, M, M] the trial's G (afq_thermal_reset)
    double *th_stack = nullptr;     // [nw, nbins, 2, M, M]
    double *th_u = nullptr;         // [nw, M] uniforms of the slice
    int *th_fields = nullptr;       // [nw, M] chosen fields (-1: both probabilities vanished)
    double *th_nav = nullptr;       // [nw]
    // continuous fields (k_thermal_cplx.hip; thermal_propagation/planewave.py, continuous.py with hubbard.py:199-250): the
    // walker's matrices are complex, thc_* are its state
    cplx *thc_G = nullptr;          // [nw, 2, M, M]
    cplx *thc_G0 = nullptr;         // [2, M, M] the trial's G
    cplx *thc_stack = nullptr;      // [nw, nbins, 2, M, M]
    cplx *thc_right = nullptr;      // [nw, 2, M, M] product of the slices of the current bin
    cplx *thc_M0 = nullptr;         // [nw, 2] det G_s the weight update divides by
    cplx *thc_M00 = nullptr;        // [2] the trial's
    cplx *thc_det = nullptr;        // [nw, 2] det G_s of the last evaluation
    cplx *thc_mf = nullptr;         // [K] mean-field shift
    double thc_fb_bound = 1.0;      // |xbar_i| above it is scaled to unit modulus
    // the trial's tables: diagonals [.., 2, M] with a diagonal trial (UEG), full matrices [.., 2, M, M] with a dense one
    double *thc_BTpow = nullptr;    // BT^stack_size
    double *thc_left = nullptr;     // [stack_size, ..] left_k = BT^stack_size BT_inv^(k + 1)
    double *thc_bh1 = nullptr;      // BH1
    // the dense trial's alone (afq_thermal_configure_hubbard_continuous)
    double thd_mf_const[2] = {1.0, 0.0};   // exp(-dt mf_core) (re, im)
    double thd_sqrt_u = 0.0;        // iu_fac = i sqrt(U)
    // afq_thermal_estimates (k_thermal.hip): the sweep's chunk of G, P and (streamed) T, taken in whole bins under
    // th_sw_budget bytes (0: the default), and its small results (energies, nav, the sums); both grown on demand
    unsigned char *th_sw_ws = nullptr, *th_sw_out = nullptr;
    size_t th_sw_ws_len = 0, th_sw_out_len = 0, th_sw_budget = 0;

    // ---- propagator
    bool have_prop = false;
    cplx *BH1 = nullptr;            // [2, M, M]
    double cap_frac = 0.0, cap_total = -1.0;   // afq_set_weight_cap: cap applied inside the weight-update kernel
    bool bh1_same = false;          // BH1[0] and BH1[1] are bitwise equal
    bool bh1_real = false;          // every imaginary part of BH1 is exactly zero (real trial, real L_n)
    cplx *mf_shift = nullptr;       // [K]
    double dt = 0.0, sqrt_dt = 0.0;
    int exp_order = 6;
    int flags = AFQ_PROP_HYBRID | AFQ_PROP_FORCE_BIAS;
    int nv = 1;                     // VHS matrices per walker (2 for Hubbard spin HS)
    bool vhs_diag = false;          // Hubbard: VHS stored as diagonals [nw, nv, M]

    // ---- walkers
    int nw = 0;
    cplx *phi = nullptr;            // [nw, M, nt]
    cplx *phi_t = nullptr;          // scratch [nw, M, nt] (Taylor term ping)
    cplx *phi_t2 = nullptr;         // scratch [nw, M, nt] (Taylor term pong)
    double *weight = nullptr, *unscaled = nullptr, *detR = nullptr;
    // use_log_shift (walkers/handler.py:45,456-475): the shifts are the same for every walker, log_detR is per walker
    double *log_detR = nullptr;     // [nw]
    bool log_shift_on = false;
    double log_shift = 0.0, detR_shift = 0.0;
    cplx *ot = nullptr, *ehyb = nullptr, *phase = nullptr, *eloc = nullptr;
    cplx *ghalf = nullptr;          // [nw, nt, M]
    cplx *G = nullptr;              // [nw, 2, M, M] (allocated on demand)
    cplx *ovlp_old = nullptr, *ovlp_new = nullptr;   // [nw]
    double *xi = nullptr;           // [nw, K]
    int fb_split = 1;               // contraction slices of the force-bias GEMM
    cplx *vbias = nullptr;          // [fb_split*2, nw, K] partial per-spin Coulomb vectors X_a, X_b
    cplx *ghalf_sum = nullptr;      // [nw, na*M] Ghalf_a + Ghalf_b when both spins share rchol (force bias on half the contraction)
    cplx *gdiag = nullptr;          // Hubbard: diag(G_s) as partial sums over row blocks of Ghalf, [2 nw, gdiag_parts, M]
    int gdiag_parts = 0;
    GreensCache gf;                 // what ghalf / ghalf_sum / gdiag / vbias / ovlp_new hold for the current walkers
    StepState step;                 // the fused step: switches, host-made operands, hand-over, transients, counts (step_state.h)
    cplx *xbar = nullptr, *xs = nullptr;              // [nw, K]
    cplx *cmf = nullptr, *cfb = nullptr;              // [nw]
    cplx *vhs = nullptr;            // [nw, nv, M, M] or [nw, nv, M] when vhs_diag
    cplx *lu_ws = nullptr;          // [nw, N, N] workspace of the generic Green's kernel (N > 128)
    cplx *big_ws = nullptr;         // [2 nw, N, N] overlap matrices / inverses (k_bigdet.hip)
    cplx *big_ws2 = nullptr;        // [2 nw, N, N] second workspace (Cholesky-QR)
    cplx *detm = nullptr;           // [2 nw] determinant mantissas
    int *dete = nullptr;            // [2 nw] determinant exponents
    double *qr_logd = nullptr;      // [2, 2 nw] log det R per Cholesky-QR pass
    int *qr_fail = nullptr;         // [nw] Cholesky breakdown -> Gram-Schmidt fallback
    cplx *energy = nullptr;         // [nw, 3]
    cplx *exx_part = nullptr;       // exchange partial sums
    size_t exx_part_len = 0;
    double *gfrag = nullptr;        // Ghalf in MFMA fragment order (energy kernel B operand)
    size_t gfrag_len = 0;
    bool prop_pending = false;                      // afq_propagate_begin done, afq_propagate_finish outstanding
    double *est_stage = nullptr;                    // mapped host memory: estimator sums + scal[4] + sequence number
    unsigned long long est_seq = 0;
    double scal_cache[AFQ_NSCAL] = {0};   // scal[] as of the last afq_estimates_get_end; stale after a population control
    bool scal_cache_valid = false;
    bool est_pending = false;
    unsigned ktrace_mask = 0;          // bit k: event pairs around the launches of kernel kind k
    std::vector<hipEvent_t> ktrace_ev[AFQ_K_COUNT];   // start/stop pairs
    double issued_flops[AFQ_K_COUNT] = {0, 0, 0, 0, 0};   // matrix-pipe flops of the last launch of each kind (afq_kernel_issued_flops)
    int ktrace_used[AFQ_K_COUNT] = {0, 0, 0, 0, 0};
    int ktrace_stride[AFQ_K_COUNT] = {1, 1, 1, 1, 1}, ktrace_seen[AFQ_K_COUNT] = {0, 0, 0, 0, 0};   // every n-th launch of a kind is timed
    // afq_launch_trace: an event pair around EVERY launch, keyed by the launch's breadcrumb name (a profile pass, not
    // something to leave on inside a timed region)
    bool ltrace_on = false, ltrace_open = false;
    std::vector<hipEvent_t> ltrace_ev;
    std::vector<const char *> ltrace_name;
    int *gj_flag = nullptr;         // [2 nw] blocked Gauss-Jordan: 1 = a pivot block was poorly conditioned (k_bigdet.hip)
    cplx *estimates = nullptr;      // [10]
    // Mixed estimator with one_rdm: True (estimators/mixed.py:226-229): G then is per-walker STATE (walker.G: the
    // Green's function the walker last evaluated -- before the step's propagation, or at an energy evaluation),
    // cloned by the comb, and rdm_acc += sum_w weight_w Re G_w with every afq_estimates_update
    bool rdm_on = false;
    double *rdm_acc = nullptr;      // [2, M, M]
    // Mixed estimator with two_rdm: 'structure_factor' (afq_estimates_sf): sf_acc += sum_w weight_w Re two_rdm[G_w] with
    // every afq_estimates_update that evaluates the energy
    bool sf_on = false;
    double *sf_acc = nullptr;       // [2, 2, nq]
    unsigned long long *counters = nullptr;   // [AFQ_NCOUNTERS]
    int *alive = nullptr;           // [nw]
    int *parent_ix = nullptr;       // [nw]
    // [AFQ_NSCAL] device scalars: 0 total weight of the last comb, 1 local pairs (< 0: collapsed), 2 collapse flag (sticky),
    // 3 exchange overflow (sticky), 4 largest transfer between two ranks, 5 comb events, 6 communication error (sticky:
    // a peer's flag never arrived), 7 walkers this rank has sent, 8 bytes this rank has sent (window transport)
    // 9 uniforms the last pair-branch event consumed
    double *scal = nullptr;
    void *pack_tmp = nullptr;
    double *pb_u = nullptr;         // [pb_u_n] the uniforms of afq_popcontrol_pair_branch, staged for its plan kernel
    size_t pb_u_n = 0;
    void *zero_page = nullptr;      // 256 zero bytes: source of out-of-range LDS-DMA loads
    // afq_estimates_fuse_next: the weight update of the next step adds every walker's estimator terms to est_acc[w][6]
    // (per walker: no cross-walker sum, no atomics); the next estimates_kernel launch, or the next fetch, folds them in
    double *est_acc = nullptr;
    bool fuse_est_req = false, est_acc_pending = false;

    // rng
    uint64_t rng_seed = 0, rng_stream = 0, rng_counter = 0;
    bool rng_inline = false;            // this step's fields are drawn inside fields_kernel (no rng launch)
    uint64_t rng_inline_counter = 0;

    // diagnostics: host-side breadcrumbs of the launches queued on the stream (afq_last_launch)
    const char *crumb_name[64] = {nullptr};     // ring of the last 64 kernel names (string literals)
    const char *crumb_api = "";                 // C-ABI entry point that queued them
    volatile unsigned long long n_launch = 0;   // launches queued so far
    bool debug_sync = false;                    // AFQ_DEBUG_SYNC=1: synchronise + check after every launch
    bool debug_markers = false;                 // AFQ_DEBUG_MARKERS=1: a 1-thread marker kernel behind every launch
    volatile unsigned long long *retired = nullptr;   // pinned, device-mapped: index of the last RETIRED launch

    // library-owned RCCL communicator (afq_comm_init; walkers/handler.py:232,291,313,322, mixed.py:261,273)
    void *comm = nullptr;                       // afq_comm_state (k_comm.hip)

    // timers
    bool timers_on = false;
    double t_ms[T_COUNT] = {0};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double last_energy_ms = 0.0;
};

// An entry point that rewrites phi, the trial or the propagator: neither the cached Green's function nor the step hand-over
// describes the walkers any more
inline void drop_walk_caches(afq_handle *h) { if (h) { h->gf.drop(); h->step.handover.drop(); } }

inline bool th_thermal(const afq_handle *h) { return h->th_kind != TH_NONE; }
inline bool th_complex(const afq_handle *h) { return h->th_kind == TH_CPLX_DIAG || h->th_kind == TH_CPLX_DENSE; }
// AFQ_THERMAL_DELAYED: the real walkers on the wide engine take the delayed slice kernel
inline bool th_delayed_slice(const afq_handle *h) { return h->th_kind == TH_REAL && h->th_engine == TH_ENGINE_WIDE; }

#define AFQ_HIP(h, call)                                                        \
    do {                                                                        \
        hipError_t e_ = (call);                                                 \
        if (e_ != hipSuccess) {                                                 \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);       \
            return AFQ_EHIP;                                                    \
        }                                                                       \
    } while (0)

// every kernel launch goes through AFQ_LAUNCH / AFQ_GEMM + AFQ_POST: the name of the kernel is left in the
// handle's breadcrumb ring before the launch, and AFQ_POST checks the launch (and, in the debug modes,
// queues a marker or synchronises so that a failing or hanging kernel is identified by name)
void afq_launch_trace_mark(afq_handle *h, const char *name);      // afq_api.hip
inline void afq_note_launch(afq_handle *h, const char *name) {
    h->crumb_name[h->n_launch & 63] = name;
    h->n_launch = h->n_launch + 1;
    if (h->ltrace_on) afq_launch_trace_mark(h, name);
}
hipError_t afq_post_launch(afq_handle *h);      // afq_api.hip
#define AFQ_LAUNCH(h, kern, ...) do { afq_note_launch((h), #kern); hipLaunchKernelGGL(kern, __VA_ARGS__); } while (0)
#define AFQ_POST(h)                                                              \
    do {                                                                        \
        hipError_t e_ = afq_post_launch(h);                                     \
        if (e_ != hipSuccess) {                                                 \
            (h)->err = std::string("kernel ") + (h)->crumb_name[((h)->n_launch - 1) & 63] + ": " + hipGetErrorString(e_); \
            return AFQ_EHIP;                                                    \
        }                                                                       \
    } while (0)
#define AFQ_GEMM(h, call) AFQ_GEMM_AS(h, __func__, call)
// the same with the breadcrumb / launch-trace name chosen by the caller (functions that launch several different GEMMs)
#define AFQ_GEMM_AS(h, name, call)                                              \
    do {                                                                        \
        afq_note_launch((h), name);                                             \
        hipError_t e_ = (call);                                                 \
        if (e_ == hipSuccess) e_ = afq_post_launch(h);                          \
        if (e_ != hipSuccess) {                                                 \
            (h)->err = std::string("GEMM of ") + __func__ + ": " + hipGetErrorString(e_); \
            return AFQ_EHIP;                                                    \
        }                                                                       \
    } while (0)

// hipFuncAttributeMaxDynamicSharedMemorySize is per (kernel, device): raise it once per device
#define AFQ_MAX_DEVICES 16
inline hipError_t afq_raise_lds(const void *kern, size_t lds, size_t (&set)[AFQ_MAX_DEVICES]) {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= AFQ_MAX_DEVICES) d = -1;
    if (d >= 0 && lds <= set[d]) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess && d >= 0) set[d] = lds;
    return e;
}

#define AFQ_FAIL(h, code, msg) do { (h)->err = (msg); return (code); } while (0)
#define AFQ_TRY(call) do { if (int rc_ = (call)) return rc_; } while (0)     // (the callee has set err)

// ---- the three ways a handle field comes to own device memory (dev_mem.h); what names the failing buffer in the error
// allocate or replace: n elements (0: the slot stays null)
inline int dev_nomem(afq_handle *h, const char *what, size_t bytes, hipError_t e) {
    (void)hipGetLastError();
    h->err = std::string(what) + ": hipMalloc of " + std::to_string(bytes) + " bytes failed (" + hipGetErrorString(e) + ")";
    return AFQ_ENOMEM;
}
template <class T> static int dev_alloc(afq_handle *h, Lifetime lt, T **p, size_t n, const char *what = "device buffer",
                                        size_t *len = nullptr) {
    const hipError_t e = h->mem.replace(lt, (void **)p, n * sizeof(T), len, DevFloating<T>::value, what);
    return e == hipSuccess ? AFQ_OK : dev_nomem(h, what, n * sizeof(T), e);
}
template <class T> static int dev_upload(afq_handle *h, Lifetime lt, T **p, const void *src, size_t n,
                                         const char *what = "device buffer") {
    int rc = dev_alloc(h, lt, p, n, what);
    if (rc) return rc;
    if (n) AFQ_HIP(h, hipMemcpy(*p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return AFQ_OK;
}
// ensure: allocate if the slot is null (a block of this lifetime is never of another size)
template <class T> static int dev_ensure(afq_handle *h, Lifetime lt, T **p, size_t n, const char *what = "device buffer") {
    return *p ? AFQ_OK : dev_alloc(h, lt, p, n, what);
}
// grow: at least n elements; queued work may still read the block that is freed.  Failure leaves null and *len == 0.
template <class T> static int dev_grow(afq_handle *h, Lifetime lt, T **p, size_t *len, size_t n, const char *what) {
    if (n <= *len) return AFQ_OK;
    if (*p) hipStreamSynchronize(h->stream);
    const int rc = dev_alloc(h, lt, p, n, what, len);
    if (!rc) *len = n;
    return rc;
}

// a per-call buffer (freed when its DevTemp leaves scope), filled from the host when src is given
template <class T> static int dev_temp(afq_handle *h, DevTemp<T> &t, size_t n, const void *src = nullptr) {
    const hipError_t e = t.alloc(n, &h->mem);
    if (e != hipSuccess) return dev_nomem(h, "per-call buffer", n * sizeof(T), e);
    if (src) AFQ_HIP(h, hipMemcpy(t.p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return AFQ_OK;
}

// the handle's trial operands become views of dets[d] (and ghalf / vbias its slices)
inline void select_det(afq_handle *h, int d, bool refresh = false) {
    if (d == h->cur_det && !refresh) return;
    const afq_handle::DetOps &o = h->dets[d];
    h->psi = o.psi; h->psic = o.psic; h->rH1 = o.rH1; h->rchol_re = o.rchol_re; h->rchol_im = o.rchol_im;
    for (int s = 0; s < 2; ++s) { h->rchol_frag[s] = o.rchol_frag[s]; h->rchol_frag_im[s] = o.rchol_frag_im[s]; h->atil[s] = o.atil[s]; }
    h->rchol_same = o.rchol_same;
    h->cur_det = d;
    if (h->nw) {
        h->ghalf = h->ghalf_all + (size_t)d * h->nw * h->M * h->nt;
        if (h->vbias_all) h->vbias = h->vbias_all + (size_t)d * 2 * h->fb_split * h->nw * h->K;
    }
}

struct PhaseTimer {
    afq_handle *h; int slot;
    PhaseTimer(afq_handle *h_, int s) : h(h_), slot(s) {
        if (h->timers_on) hipEventRecord(h->ev0, h->stream);
    }
    ~PhaseTimer() {
        if (h->timers_on) {
            hipEventRecord(h->ev1, h->stream);
            hipEventSynchronize(h->ev1);
            float ms = 0; hipEventElapsedTime(&ms, h->ev0, h->ev1);
            h->t_ms[slot] += ms;
        }
    }
};

// Lends a handle field for a scope: the k_* launchers read their operands from the handle, so code that has them work
// on something else overwrites the field here, and every way out of the scope puts the old value back.
template <class T> struct Lent {
    T &slot; T saved;
    Lent(T &s, T v) : slot(s), saved(s) { slot = v; }
    ~Lent() { slot = saved; }
    Lent(const Lent &) = delete;
    Lent &operator=(const Lent &) = delete;
};

// Brackets ONE kernel launch with a start/stop event pair on the handle's stream when
// afq_kernel_trace is on; nothing is synchronised here (afq_kernel_trace_get reads the pairs).
struct KernelTrace {
    afq_handle *h; int kind, idx;
    KernelTrace(afq_handle *h_, int k) : h(h_), kind(k), idx(-1) {
        if (!(h->ktrace_mask >> k & 1) || h->ktrace_used[k] >= 4096) return;
        if (h->ktrace_seen[k]++ % h->ktrace_stride[k]) return;
        idx = h->ktrace_used[k];
        std::vector<hipEvent_t> &ev = h->ktrace_ev[k];
        while ((int)ev.size() < 2 * idx + 2) { hipEvent_t e; hipEventCreate(&e); ev.push_back(e); }
        hipEventRecord(ev[2 * idx], h->stream);
    }
    ~KernelTrace() {
        if (idx < 0) return;
        hipEventRecord(h->ktrace_ev[kind][2 * idx + 1], h->stream);
        h->ktrace_used[kind] = idx + 1;
    }
};

// ---- launchers implemented in the kernel translation units -----------------
// k_gemm.hip
int k_onebody(afq_handle *h, const cplx *rowscale = nullptr);   // phi <- [diag(rowscale_w)] BH1 phi (all live walkers)
int k_force_bias_generic(afq_handle *h);                    // ghalf -> vbias[2,nw,K]
bool k_msd_vbias_current(afq_handle *h);                    // every determinant's force-bias partials are current
bool k_msd_gbar_wanted(afq_handle *h);                      // multi-determinant force bias through the averaged G
int k_force_bias_msd_gbar(afq_handle *h);                   // ghalf_all, detw -> averaged partials in vbias_all
bool k_fb_use_sum(afq_handle *h);                           // force bias runs once over Ghalf_a + Ghalf_b
int k_vhs_generic(afq_handle *h);                           // xs -> vhs
int k_apply_exponential(afq_handle *h, const cplx *vhs);    // phi <- sum_n vhs^n/n! phi
int k_full_G(afq_handle *h);                                // G = conj(psi) ghalf
// k_fused.hip: reads of the launch plan (step_plan.h) made of the handle as it is
int k_prop_fused_supported(afq_handle *h);
int k_prop_closed_resident(afq_handle *h);                  // closed walkers take the body with V resident in registers
bool k_step_fuses(afq_handle *h);                           // THIS step runs its closing Green's function as the tail
struct GreensLaunch;
// phi <- B exp(V) B phi for live walkers, in place; with `tail` (k_prop_fused_greens, k_small.hip) the Green's function, overlap and weight
// update of EVERY walker's new phi behind it in the same launch, the resident closed-shell body with 3-multiplication Taylor
// products when mul3
int k_prop_fused(afq_handle *h, const GreensLaunch *tail = nullptr, bool mul3 = false);
// k_hirsch.hip
int k_hirsch_alive(afq_handle *h, int mode);
int k_hirsch_kinetic(afq_handle *h);
int k_hirsch_two_body(afq_handle *h);
int k_hirsch_eshift(afq_handle *h, double fac);
int k_hirsch_free(afq_handle *h, double eshift);           // free-projection step from the uniforms in hs_u
int k_rng_uniform(afq_handle *h, double *u, long n);
// k_fullg.hip
int k_energy_full_g(afq_handle *h, const cplx *G_dev, int ng, cplx *E_dev);   // estimators/generic.py:398-434
int k_fullg_expand(afq_handle *h);                         // L_full (real vectors) built on first use
// k_bp_obs.hip: sum_w wt_w two_rdm[G_bp[w]] -> two_out [M^4], sum_w wt_w (F1p, F1h)[G_bp[w]] -> fock_out [2, M, M]
// (either may be null); after afq_bp_update's accumulation, before its reset
int k_bp_observables(afq_handle *h, int restore, cplx *two_out, cplx *fock_out);
// k_itcf.hip: the pieces of one imaginary-time Green's function window (afq_itcf_update)
int k_itcf_fields(afq_handle *h, cplx *xs, int t);           // xs[w] = recorded fields of window step t
int k_itcf_generic_b(afq_handle *h, const cplx *vhs, const cplx *BT2, const cplx *BT2inv, cplx *B, cplx *Binv, cplx *ws,
                     cplx *detm, int *dete);                 // B, B^-1 [nw, 2, M, M] of the VHS [nw, M, M]
int k_itcf_hirsch_b(afq_handle *h, int t, const cplx *BT2, const cplx *BT2inv, cplx *B, cplx *Binv, double *f);
int k_itcf_mul(afq_handle *h, const cplx *A, const cplx *B, cplx *C);                // C = A B per (walker, spin)
int k_itcf_propagate(afq_handle *h, const cplx *B, const cplx *src, cplx *dst);     // dst = B src per spin block
int k_itcf_projectors(afq_handle *h, const cplx *G, cplx *P, cplx *Q);              // P = G^T, Q = I - P
int k_itcf_weights(afq_handle *h, int restore, cplx *wfac, cplx *denom);
int k_itcf_accumulate(afq_handle *h, const cplx *Ggr, const cplx *Gls, const cplx *wfac, cplx *spgf_tau);
// k_bigdet.hip
int k_greens_big_supported(afq_handle *h);
// ghalf may be null (overlap only); req as launch_greens (k_small.hip) has narrowed it: ride_weight is taken as decided
int k_greens_big(afq_handle *h, cplx *ghalf, cplx *det, cplx *oinv, const GreensRequest &req, GreensResult *res);
int k_reortho_big(afq_handle *h);                           // Cholesky-QR2; sets qr_fail for breakdowns
int k_gj_inverse(afq_handle *h, cplx *O, int n, int batch, cplx *detm, int *dete);   // in place, n <= 128
// k_small.hip
int k_alive(afq_handle *h);
int k_greens(afq_handle *h, cplx *det_out, const GreensRequest &req = GreensRequest(), GreensResult *res = nullptr);   // ghalf + det
int k_overlap(afq_handle *h, cplx *det_out, const GreensRequest &req = GreensRequest(), GreensResult *res = nullptr);  // det(psi^H phi)
int k_inverse_overlap(afq_handle *h, cplx *oinv, cplx *det_out);   // O^-1 [nw,2,nmax,nmax] + det, live walkers
int k_fields(afq_handle *h);                                // vbias -> xbar(clipped), xs, cmf, cfb
int k_fields_explicit(afq_handle *h, const double *xi_d, const cplx *xbar_d, cplx *xs_d, cplx *cmf_d, cplx *cfb_d);
int k_xbar(afq_handle *h);                                 // vbias / G -> xbar (unclipped), system dispatch
int k_bp_push(afq_handle *h);
int k_bp_fields(afq_handle *h, int i);
int k_bp_init(afq_handle *h, const cplx *phi0_dev);
int k_conj_copy(afq_handle *h, const cplx *src, cplx *dst, long n);
int k_conj_transpose(afq_handle *h, const cplx *A, cplx *At);
int k_bp_accumulate(afq_handle *h, int restore, int with_energy);
int k_bp_reset(afq_handle *h, bool first);
int k_bp_hirsch_step(afq_handle *h, int i);                 // B(x)^H of the i-th most recent discrete configuration
// k_bp_msd.hip: the backward pass and the determinant-weighted sums of a multi-determinant window (afq_bp_update_msd).
// The column-stacked products take phi as [ndet, nw, M, nt] and every walker's BH1^H / V once for its ndet nt columns.
int k_bp_msd_onebody(afq_handle *h, int ndet, const cplx *src, cplx *dst);              // dst[d, w] = BH1[s] src[d, w]
int k_bp_msd_taylor(afq_handle *h, int ndet, const cplx *vhs, cplx *phi, cplx *t0, cplx *t1);   // phi <- sum_n V^n / n! phi
int k_bp_msd_logr(afq_handle *h, const double *detR, double *logr, long n);            // logr += log det R
int k_bp_msd_detw(afq_handle *h, int ndet, int d, const cplx *coeffs, const double *logr, const cplx *ovlp, cplx *detw,
                  cplx *S);                                                            // w_d and S (+)= w_d
int k_bp_msd_gsum(afq_handle *h, int ndet, int d, const cplx *detw, const cplx *G, cplx *gsum, const cplx *E, cplx *esum);
int k_bp_msd_finish(afq_handle *h, int ndet, int restore, cplx *detw, const cplx *S, cplx *fac);
int k_bp_msd_accumulate(afq_handle *h, const cplx *gsum, const cplx *fac, const cplx *esum, cplx *est);
int k_xbar_fields(afq_handle *h, cplx *hubbard_factors = nullptr);   // + the Hubbard row-scaling factors (continuous fields)
int k_msd_combine(afq_handle *h, cplx *det_out, bool skip_small);          // detd -> detw, det_out = sum_d detw
int k_msd_energy_combine(afq_handle *h);                   // energy_all, detw -> energy
int k_update_weight(afq_handle *h, cplx eshift);
struct WeightArgs;
WeightArgs k_weight_args(afq_handle *h, cplx eshift);       // the weight update's operands, for the kernels it rides on
// the fused propagator with the step's closing Green's function (k_greens into ovlp_new, as req asks) as the tail of its launch
int k_prop_fused_greens(afq_handle *h, const GreensRequest &req, GreensResult *res, bool mul3);
int k_reortho(afq_handle *h, cplx *keep = nullptr, bool *keep_done = nullptr);
int k_cap_weights(afq_handle *h, double frac, double total_weight);
int k_comb(afq_handle *h, double r, double target, bool with_greens = false);
// single-rank pair branching: plan from the uniforms u_dev[nw / 2] (device), then the clones; weights are not reset
int k_pair_branch(afq_handle *h, const double *u_dev, double target, double min_weight, double max_weight,
                  bool with_greens = false);
int k_clone_pairs(afq_handle *h, bool with_greens, bool reset_weights = false);
int k_closed_flags(afq_handle *h);          // closed_w[w] for every walker
int k_closed_copy_beta(afq_handle *h);      // phi[w][:, na:] = phi[w][:, :na] where closed_w[w]
int k_scale_by_inverse(afq_handle *h, cplx *x, const double *d);   // x[w] /= d[w]
int k_log_shift_reortho(afq_handle *h);                            // detR -> exp(log det R - detR_shift), log_detR += log
int k_log_ovlp_sums(afq_handle *h, double *out3);                  // sums of |ot|, |detR|, |log_detR| (device -> host)
int k_scale_weights(afq_handle *h, double scale);
int k_reset_weights(afq_handle *h, bool after_comb = false);
// the hand-over of a block's sums to the host (afq_estimates_get_begin): written into mapped host memory, zeroed, sequence
// number published -- by est_publish_kernel, or by the estimates_kernel launch that folds the last accumulators in (host_out
// null: no hand-over)
struct EstPublish {
    double *host_out = nullptr;
    unsigned long long *host_seq = nullptr;
    unsigned long long seq = 0;
    const double *scal = nullptr;
    const unsigned long long *closed_bad = nullptr;
    int nest = 0, zero = 0;
};
int k_estimates(afq_handle *h, int have_energy, bool fold_only = false, const EstPublish *pub = nullptr);
int k_rdm_accumulate(afq_handle *h);
int k_rng_normal(afq_handle *h);
int k_rng_normal_into(afq_handle *h, double *out_d, long n);
int k_philox_raw(afq_handle *h, const unsigned int *in_d, unsigned int *out_d, int n);
// k_ueg.hip (plane-wave step from Ghalf and per-walker HS coefficients: no G, no dense HS potential)
int k_ueg_fast_system(afq_handle *h, int M, int nq, const int64_t *Acp, const int64_t *Arow, const double *Aval,
                      const int64_t *Bcp, const int64_t *Brow, const double *Bval);
int k_ueg_fast_trial(afq_handle *h, const double *psi);
int k_ueg_fast_propagator(afq_handle *h, const double *BH1);
int k_ueg_fast_supported(afq_handle *h);
int k_ueg_fields(afq_handle *h);                            // force bias + fields + HS coefficients
int k_prop_ueg(afq_handle *h);                              // phi <- B exp(V) B phi
int k_ueg_step(afq_handle *h);                              // the two above in one launch when its LDS plan fits
void k_ueg_fast_free(afq_handle *h);
// k_comm.hip
int k_comm_size(afq_handle *h);                             // ranks of the library-owned communicator (1 without)
void k_comm_destroy(afq_handle *h);
int k_comm_popcontrol(afq_handle *h, double r, double target, bool with_greens);
// k_energy.hip
int k_energy_generic(afq_handle *h);
int k_prepare_energy_operands(afq_handle *h, const double *rchol_host);
int k_exchange_uses_quadratic(afq_handle *h);            // which algorithm k_energy_generic takes for the current trial
// k_models.hip (Hubbard / UEG)
int k_vhs_hubbard(afq_handle *h);
int k_apply_exponential_diag(afq_handle *h, const cplx *vhs_diag);
int k_exp_diag_factors(afq_handle *h, const cplx *vhs_diag, cplx *out);   // out[w, v, p] = sum_{n <= order} d^n / n!
int k_energy_hubbard(afq_handle *h);
int k_vbias_ueg(afq_handle *h);
int k_vhs_ueg(afq_handle *h);
int k_energy_ueg(afq_handle *h);
// k_ueg_sf.hip: the UEG pair sums per momentum transfer on general Green's functions G_dev [n, 2, M, M] ->
// E_dev [n, 3] (no ecore), two_dev [n, 2, 2, nq]; their weighted sum over n in index order; the Hubbard energy of full G
int k_ueg_pair_mode(afq_handle *h);                          // 0 spin block in LDS, 1 the lists' rows in LDS, 2 global
int k_ueg_pair_sums(afq_handle *h, const cplx *G_dev, int n, cplx *E_dev, cplx *two_dev);
int k_ueg_sf_two(afq_handle *h, int n, cplx **two_dev, cplx **E_dev);   // the handle's [n, 2, 2, nq] + [n, 3] scratch
int k_ueg_sf_wsum(afq_handle *h, const cplx *two_dev, int n, const cplx *wt_c, const double *wt_r, cplx *out_c,
                  double *acc_r);                            // out_c = sum_g wt[g] two[g]; acc_r += Re of it
int k_energy_hubbard_full_g(afq_handle *h, const cplx *G_dev, int n, cplx *E_dev);   // estimators/hubbard.py:93-114
// k_thermal.hip
int k_thermal_greens(afq_handle *h, int slice_ix);          // th_G of every walker from its stack
// k_thermal_cplx.hip
int k_thermal_c_greens(afq_handle *h, int slice_ix);        // thc_G and thc_det of every walker from its stack
int k_thermal_c_reset(afq_handle *h, bool with_m0);         // with_m0: M0 <- the trial's (a fresh population)
int k_thermal_c_energy(afq_handle *h, double *E_out, double *nav_out);
// the sweep of afq_thermal_estimates on the complex walkers: G of nb bins from ts0 on into Gs (Ts: the streamed engine's
// scratch), then P and nav of those nb nw Green's functions
int k_thermal_c_sweep_greens(afq_handle *h, cplx *Gs, cplx *Ts, int ts0, int nb);
int k_thermal_c_sweep_rdm(afq_handle *h, const cplx *Gs, cplx *P, double *nav, int n);
// k_corr.hip: <n_is n_jt> and <S+_i S-_j> of full Green's functions G_dev [n, 2, M, M] -> out_dev [n, 5, M, M], and
// their weighted sum over n -> out_dev [5, M, M] (Green's functions of weight zero left out), in index order
int k_corr_full_g(afq_handle *h, const cplx *G_dev, int n, cplx *out_dev);
int k_corr_wsum(afq_handle *h, const cplx *G_dev, int n, const cplx *wt_c, cplx *out_dev);
int k_sum_chunks(afq_handle *h, const cplx *part, int nchunk, size_t len, cplx *out_dev);   // out[e] = sum_c part[c][e], in chunk order
// k_pair.hip: <D+(i, nbr[b][i]) D(j, nbr[b'][j])> over the handle's bond table (pair_nbr, pair_nb >= 1) of full Green's
// functions G_dev [n, 2, M, M] -> out_dev [n, nb, nb, M, M], and their weighted sum over n -> out_dev [nb, nb, M, M]
// (Green's functions of weight zero left out), in index order
int k_pair_full_g(afq_handle *h, const cplx *G_dev, int n, cplx *out_dev);
int k_pair_wsum(afq_handle *h, const cplx *G_dev, int n, const cplx *wt_c, cplx *out_dev);
