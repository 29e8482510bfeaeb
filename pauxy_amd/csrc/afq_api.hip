// C ABI of libafqmc_hip.so (see include/afqmc_hip.h): handle lifetime, uploads of
// the read-only inputs, walker storage, and the sequencing of the kernels that
// make up one propagation step (propagation/continuous.py:232-262).
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "afq_host.h"
#include "walker_fields.h"

namespace {

// ---- the three releases below free by lifetime (dev_mem.h); what stays next to them are the resets that are not memory
void free_dets(afq_handle *h) {
    h->mem.release(LT_TRIAL);
    h->dets.assign(1, afq_handle::DetOps());
    h->ndet = 1;
    select_det(h, 0, true);
    h->msd_fb_gbar = false;
}

void free_system(afq_handle *h) {
    free_dets(h);
    h->mem.release(LT_SYSTEM);
    h->hs_cplx = 0; h->sf_nlong = 0; h->kind = 0; h->pair_nb = 0;
    h->hirsch = false;              // the discrete propagator belongs to the system it was set for
}

void free_walkers(afq_handle *h) {
    h->mem.release(LT_WALKERS);
    h->ghalf = nullptr; h->vbias = nullptr;         // views of ghalf_all / vbias_all
    h->est_acc_pending = false; h->fuse_est_req = false;
    h->gf.gsum.clear(); h->gf.vbias.clear(); h->gf.gdiag.clear(); h->gdiag_parts = 0;
    h->msd_fb_gbar = false;
    h->nbp = 0; h->bpo_two = h->bpo_ekt = h->bpo_sf = h->bpo_corr = h->bpo_pair = 0; h->bpo_nL = 0; h->it_nmax = 0;
    h->rdm_on = false; h->sf_on = false;
    h->th_kind = TH_NONE; h->th_engine = TH_ENGINE_RESIDENT;
    h->nw = 0;
}

// rH1[i, q] = sum_p conj(psi[p, i]) H1_s[p, q]  (s = spin of orbital i)
int build_rH1(afq_handle *h, const std::vector<double> &H1, const std::vector<double> &psi) {
    const int M = h->M, nt = h->nt;
    std::vector<double> r((size_t)nt * M * 2, 0.0);
    for (int i = 0; i < nt; ++i) {
        const int s = i < h->na ? 0 : 1;
        for (int p = 0; p < M; ++p) {
            const double cr = psi[((size_t)p * nt + i) * 2], ci = -psi[((size_t)p * nt + i) * 2 + 1];
            if (cr == 0.0 && ci == 0.0) continue;
            const double *hrow = &H1[(((size_t)s * M + p) * M) * 2];
            double *out = &r[(size_t)i * M * 2];
            for (int q = 0; q < M; ++q) {
                const double hr = hrow[2 * q], hi = hrow[2 * q + 1];
                out[2 * q] += cr * hr - ci * hi;
                out[2 * q + 1] += cr * hi + ci * hr;
            }
        }
    }
    int rc = dev_upload(h, LT_TRIAL, &h->dets[h->cur_det].rH1, r.data(), (size_t)nt * M);
    select_det(h, h->cur_det, true);
    return rc;
}

}  // namespace

// host copies kept for derived operands (small: H1 and psi only)
struct afq_host_cache {
    std::vector<double> H1, psi;
    std::vector<double> BH1;        // Re BH1[0] [M, M] of the last afq_set_propagator (psiB_cT is made of it and psi)
};
static afq_host_cache *cache_of(afq_handle *h);

struct afq_handle_full : afq_handle {
    afq_host_cache cache;
};
static afq_host_cache *cache_of(afq_handle *h) { return &static_cast<afq_handle_full *>(h)->cache; }

static int step_operands(afq_handle *h);

static int upload_psi(afq_handle *h, const double *psi) {
    const size_t n = (size_t)h->M * h->nt;
    afq_handle::DetOps &o = h->dets[h->cur_det];
    int rc = dev_upload(h, LT_TRIAL, &o.psi, psi, n);
    if (rc) return rc;
    cache_of(h)->psi.assign(psi, psi + 2 * n);
    h->psi_real = true;
    for (size_t i = 0; i < n && h->psi_real; ++i) h->psi_real = psi[2 * i + 1] == 0.0;
    h->psi_closed = h->na == h->nb && h->na > 0;
    for (int p_ = 0; p_ < h->M && h->psi_closed; ++p_)
        h->psi_closed = memcmp(psi + 2 * (size_t)p_ * h->nt, psi + 2 * ((size_t)p_ * h->nt + h->na), sizeof(double) * 2 * h->na) == 0;
    std::vector<double> pc(psi, psi + 2 * n);
    for (size_t i = 0; i < n; ++i) pc[2 * i + 1] = -pc[2 * i + 1];
    if (h->ndet <= 1) {     // transposed copy (Hubbard force bias: diag of G from rows of conj(psi)^T and Ghalf)
        std::vector<double> pt(2 * n);
        for (int p_ = 0; p_ < h->M; ++p_)
            for (int i = 0; i < h->nt; ++i) {
                pt[2 * ((size_t)i * h->M + p_)] = pc[2 * ((size_t)p_ * h->nt + i)];
                pt[2 * ((size_t)i * h->M + p_) + 1] = pc[2 * ((size_t)p_ * h->nt + i) + 1];
            }
        if ((rc = dev_upload(h, LT_TRIAL, &h->psicT, pt.data(), n))) return rc;
    }
    rc = dev_upload(h, LT_TRIAL, &o.psic, pc.data(), n);
    select_det(h, h->cur_det, true);
    return rc ? rc : step_operands(h);
}

// The fused step's operands for this trial and propagator (StepState, step_state.h): psiB_cT = psi^H B from the host copies of
// the two, after every upload of either.  Anything but a single real closed trial with one real one-body matrix for both spins
// leaves the slot null, and the fused propagator's tail then evaluates the overlap matrix itself.  B2 = B B (the step hand-over)
// is made here too, under the same conditions and in the same lifetime slot; a new trial or propagator drops the hand-over that
// was made with the old one.
static int step_operands(afq_handle *h) {
    afq_host_cache *c = cache_of(h);
    const int M = h->M, nt = h->nt, na = h->na;
    const bool ok = h->have_prop && h->ndet <= 1 && h->psi_stride == 0 && h->psi_real && h->psi_closed &&
                    h->bh1_real && h->bh1_same && c->psi.size() == (size_t)2 * M * nt && c->BH1.size() == (size_t)M * M;
    StepState &st = h->step;
    st.operands_gone();
    if (!ok) {
        const int rc0 = dev_alloc(h, LT_TRIAL, &st.B2, 0);
        return rc0 ? rc0 : dev_alloc(h, LT_TRIAL, &st.psiB_cT, 0);
    }
    std::vector<double> pb((size_t)na * M, 0.0);
    for (int m = 0; m < M; ++m)
        for (int i = 0; i < na; ++i) {
            const double p = c->psi[2 * ((size_t)m * nt + i)];
            const double *brow = &c->BH1[(size_t)m * M];
            double *out = &pb[(size_t)i * M];
            for (int k = 0; k < M; ++k) out[k] += p * brow[k];
        }
    int rc = dev_upload(h, LT_TRIAL, &st.psiB_cT, pb.data(), pb.size());
    if (rc) return rc;
    st.made_psiB(h->dets[h->cur_det].psi, h->BH1);
    // B2 = B B for the step hand-over (the next step's opening pass as (B B) S, k_fused_closed.h): extended accumulation, one
    // rounding per element
    std::vector<double> b2((size_t)M * M);
    std::vector<long double> acc(M);
    for (int m = 0; m < M; ++m) {
        std::fill(acc.begin(), acc.end(), 0.0L);
        for (int j = 0; j < M; ++j) {
            const long double x = c->BH1[(size_t)m * M + j];
            const double *brow = &c->BH1[(size_t)j * M];
            for (int k = 0; k < M; ++k) acc[k] += x * (long double)brow[k];
        }
        for (int k = 0; k < M; ++k) b2[(size_t)m * M + k] = (double)acc[k];
    }
    rc = dev_upload(h, LT_TRIAL, &st.B2, b2.data(), b2.size());
    if (!rc) st.made_B2(h->BH1);
    return rc;
}

static int maybe_build_rH1(afq_handle *h) {
    afq_host_cache *c = cache_of(h);
    if (h->kind == 0 || !h->have_trial || c->H1.empty()) return AFQ_OK;
    return build_rH1(h, c->H1, c->psi);
}

__global__ void afq_marker_kernel(volatile unsigned long long *retired, unsigned long long n) { *retired = n; }

// afq_launch_trace: one event at the head of every launch (name != nullptr) and one behind it (name == nullptr, from
// afq_post_launch); launches queued without a post in between close their predecessor with their own head event.
void afq_launch_trace_mark(afq_handle *h, const char *name) {
    const size_t pairs = h->ltrace_name.size();
    if (name && pairs >= 65536) return;
    auto event_at = [&](size_t i) {
        while (h->ltrace_ev.size() <= i) { hipEvent_t e; hipEventCreate(&e); h->ltrace_ev.push_back(e); }
        return h->ltrace_ev[i];
    };
    if (h->ltrace_open) {            // close the launch in flight
        hipEventRecord(event_at(2 * pairs - 1), h->stream);
        h->ltrace_open = false;
    }
    if (name) {
        hipEventRecord(event_at(2 * pairs), h->stream);
        h->ltrace_name.push_back(name);
        h->ltrace_open = true;
    }
}

hipError_t afq_post_launch(afq_handle *h) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (h->ltrace_open) afq_launch_trace_mark(h, nullptr);
    if (h->debug_markers) {
        unsigned long long *dptr = nullptr;
        if (hipHostGetDevicePointer((void **)&dptr, (void *)h->retired, 0) == hipSuccess)
            hipLaunchKernelGGL(afq_marker_kernel, dim3(1), dim3(1), 0, h->stream, dptr, (unsigned long long)h->n_launch);
    }
    if (h->debug_sync) e = hipStreamSynchronize(h->stream);
    return e;
}

extern "C" {

int afq_version(void) { return 2; }

int afq_create(int device_id, afq_handle **out) {
    if (!out) return AFQ_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return AFQ_EHIP;
    if (device_id < 0 || device_id >= ndev) return AFQ_EINVAL;
    if (hipSetDevice(device_id) != hipSuccess) return AFQ_EHIP;
    afq_handle_full *h = new afq_handle_full();
    h->device = device_id;
    if (hipStreamCreate(&h->stream) != hipSuccess) { delete h; return AFQ_EHIP; }
    hipEventCreate(&h->ev0); hipEventCreate(&h->ev1);
    // AFQ_DEBUG_GUARD=1 / 2 (dev_guard.h): guard bands round every device block of this handle, and typed poison in it; read
    // before the first allocation, with the other diagnostics of the environment below
    h->mem.guard = guard_cfg_from_env();
    if (dev_alloc(h, LT_HANDLE, &h->estimates, AFQ_EST_COUNT_, "estimates") || dev_alloc(h, LT_HANDLE, &h->counters, AFQ_NCOUNTERS, "counters") ||
        dev_alloc(h, LT_HANDLE, &h->closed_bad, 1, "closed_bad") || dev_alloc(h, LT_HANDLE, &h->scal, AFQ_NSCAL, "scal") ||
        dev_alloc(h, LT_HANDLE, (char **)&h->zero_page, 256, "zero_page")) { h->mem.release(LT_HANDLE); delete h; return AFQ_ENOMEM; }
    hipMemset(h->estimates, 0, sizeof(cplx) * AFQ_EST_COUNT_);
    hipMemset(h->counters, 0, sizeof(unsigned long long) * AFQ_NCOUNTERS);
    hipMemset(h->closed_bad, 0, sizeof(unsigned long long));
    hipMemset(h->scal, 0, sizeof(double) * AFQ_NSCAL);
    hipMemset(h->zero_page, 0, 256);
    // diagnostics (not tuning): AFQ_DEBUG_SYNC=1 synchronises and checks after every launch (a failing kernel is
    // named in afq_last_error), AFQ_DEBUG_MARKERS=1 queues a marker behind every launch so that afq_last_launch
    // can tell the last launch that RETIRED apart from the last one queued
    if (hipHostMalloc((void **)&h->retired, sizeof(unsigned long long), hipHostMallocMapped) != hipSuccess) {
        delete h; return AFQ_ENOMEM;
    }
    *h->retired = 0;
    h->debug_sync = getenv("AFQ_DEBUG_SYNC") != nullptr && atoi(getenv("AFQ_DEBUG_SYNC")) != 0;
    h->debug_markers = getenv("AFQ_DEBUG_MARKERS") != nullptr && atoi(getenv("AFQ_DEBUG_MARKERS")) != 0;
    *out = h;
    return AFQ_OK;
}

int afq_destroy(afq_handle *h) {
    if (!h) return AFQ_EINVAL;
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
    k_comm_destroy(h);
    k_ueg_fast_free(h);
    free_walkers(h);
    free_system(h);
    h->mem.release(LT_HANDLE);
    if (h->retired) hipHostFree((void *)h->retired);
    hipEventDestroy(h->ev0); hipEventDestroy(h->ev1);
    if (h->est_stage) hipHostFree(h->est_stage);
    for (int k = 0; k < AFQ_K_COUNT; ++k) for (hipEvent_t e : h->ktrace_ev[k]) hipEventDestroy(e);
    for (hipEvent_t e : h->ltrace_ev) hipEventDestroy(e);
    hipStreamDestroy(h->stream);
    delete static_cast<afq_handle_full *>(h);
    return AFQ_OK;
}

// ---- AFQ_DEBUG_GUARD (dev_guard.h): the bands of every live block of the handle, and the process-wide log of violations
int afq_debug_guard_check(afq_handle *h) {
    if (!h) return AFQ_EINVAL;
    hipSetDevice(h->device);
    guard_check_owner(&h->mem);
    return AFQ_OK;
}

int afq_debug_guard_report(char *buf, int n) { return guard_report(buf, n); }

void afq_debug_guard_reset(void) { guard_reset(); }

const char *afq_last_error(afq_handle *h) { return h ? h->err.c_str() : "null handle"; }

int afq_sync(afq_handle *h) {
    if (!h) return AFQ_EINVAL;
    AFQ_HIP(h, hipStreamSynchronize(h->stream));
    return AFQ_OK;
}

int afq_stream(afq_handle *h, void **stream) {
    if (!h || !stream) return AFQ_EINVAL;
    *stream = (void *)h->stream;
    return AFQ_OK;
}

// ------------------------------------------------------------------ systems
static int set_dims(afq_handle *h, int kind, int M, int K, int na, int nb) {
    if (M <= 0 || K <= 0 || na <= 0 || nb < 0 || na > M || nb > M) AFQ_FAIL(h, AFQ_EINVAL, "bad dimensions");
    hipSetDevice(h->device);
    free_system(h);
    free_walkers(h);
    h->have_trial = false; h->have_prop = false;
    h->kind = kind; h->M = M; h->K = K; h->na = na; h->nb = nb; h->nt = na + nb;
    return AFQ_OK;
}

// half-rotated Cholesky vectors of ONE determinant into the handle's current operand slots:
// planar re / im [nt*M, ld_rc] for the force-bias GEMM + fragment-ordered copies for the exchange kernel
static bool rchol_is_real(const double *rchol, size_t n) {
    for (size_t i = 0; i < n; ++i) if (rchol[2 * i + 1] != 0.0) return false;
    return true;
}

static int upload_rchol(afq_handle *h, const double *rchol, bool real) {
    const size_t nq = (size_t)h->nt * h->M;
    const int K = h->K;
    int rc;
    std::vector<double> re(nq * h->ld_rc, 0.0);
    for (size_t q = 0; q < nq; ++q)
        for (int n = 0; n < K; ++n) re[q * h->ld_rc + n] = rchol[2 * (q * K + n)];
    h->rchol_real = real;
    h->gf.rewritten();                  // force-bias partials contracted with the old vectors are stale
    afq_handle::DetOps &o = h->dets[h->cur_det];
    o.rchol_same = h->na == h->nb && memcmp(rchol, rchol + 2 * (size_t)h->na * h->M * K, sizeof(double) * 2 * (size_t)h->na * h->M * K) == 0;
    h->atil_unavailable = false;
    if ((rc = dev_upload(h, LT_TRIAL, &o.rchol_re, re.data(), re.size()))) return rc;
    if (!real) {
        std::vector<double> im(nq * h->ld_rc, 0.0);
        for (size_t q = 0; q < nq; ++q)
            for (int n = 0; n < K; ++n) im[q * h->ld_rc + n] = rchol[2 * (q * K + n) + 1];
        if ((rc = dev_upload(h, LT_TRIAL, &o.rchol_im, im.data(), im.size()))) return rc;
    }
    select_det(h, h->cur_det, true);
    return k_prepare_energy_operands(h, rchol);
}

int afq_set_system_generic(afq_handle *h, int M, int K, int na, int nb, const double *hs_pot,
                           const double *rchol, const double *H1, double ecore) {
    drop_walk_caches(h);
    if (!h || !hs_pot || !rchol || !H1) return AFQ_EINVAL;
    int rc = set_dims(h, AFQ_SYS_GENERIC, M, K, na, nb);
    if (rc) return rc;
    h->ecore = ecore;
    const size_t mm = (size_t)M * M, nq = (size_t)h->nt * M;
    {   // hs_pot^T : [K, ld_hs] so that a VHS B-fragment is contiguous (even, zero-padded rows: the
        // LDS-DMA path moves 16-byte pairs of doubles).  Cholesky matrices of real orbitals are
        // symmetric in (p, q); then only the columns p <= q are kept and the VHS GEMM does half the work.
        bool sym = true;
        for (int p = 0; p < M && sym; ++p)
            for (int q = p + 1; q < M && sym; ++q) {
                const double *a = hs_pot + ((size_t)p * M + q) * K, *b = hs_pot + ((size_t)q * M + p) * K;
                for (int n = 0; n < K; ++n) if (a[n] != b[n]) { sym = false; break; }
            }
        h->hs_sym = sym;
        if (sym) {
            const size_t np = (size_t)M * (M + 1) / 2;
            h->ld_hs = (long)((np + 1) & ~(size_t)1);
            std::vector<double> t((size_t)K * h->ld_hs, 0.0);
            std::vector<int> pq(2 * np);
            size_t c = 0;
            for (int p = 0; p < M; ++p)
                for (int q = p; q < M; ++q, ++c) {
                    pq[2 * c] = p; pq[2 * c + 1] = q;
                    const double *a = hs_pot + ((size_t)p * M + q) * K;
                    for (int n = 0; n < K; ++n) t[(size_t)n * h->ld_hs + c] = a[n];
                }
            if ((rc = dev_upload(h, LT_SYSTEM, &h->hs_pot, t.data(), t.size()))) return rc;
            if ((rc = dev_upload(h, LT_SYSTEM, &h->hs_pair, pq.data(), np))) return rc;
        } else {
            h->ld_hs = (long)((mm + 1) & ~(size_t)1);
            std::vector<double> t((size_t)K * h->ld_hs, 0.0);
            for (size_t r = 0; r < mm; ++r)
                for (int n = 0; n < K; ++n) t[(size_t)n * h->ld_hs + r] = hs_pot[r * K + n];
            if ((rc = dev_upload(h, LT_SYSTEM, &h->hs_pot, t.data(), t.size()))) return rc;
        }
    }
    h->ld_rc = (long)((K + 1) & ~1);
    if ((rc = upload_rchol(h, rchol, rchol_is_real(rchol, nq * K)))) return rc;
    if ((rc = dev_upload(h, LT_SYSTEM, &h->H1, H1, 2 * mm))) return rc;
    cache_of(h)->H1.assign(H1, H1 + 4 * mm);
    return AFQ_OK;
}

// complex Cholesky vectors: Re and Im parts as two transposed real panels (afq_internal.h: hs_cplx)
int afq_set_system_generic_c128(afq_handle *h, int M, int K, int na, int nb, const double *hs_pot,
                                const double *rchol, const double *H1, double ecore) {
    drop_walk_caches(h);
    if (!h || !hs_pot || !rchol || !H1) return AFQ_EINVAL;
    if (M <= 0 || K <= 0) AFQ_FAIL(h, AFQ_EINVAL, "bad dimensions");
    const size_t mm = (size_t)M * M, nq = (size_t)(na + nb) * M;
    bool real = true;
    for (size_t e = 0; e < mm * K && real; ++e) real = hs_pot[2 * e + 1] == 0.0;
    if (real) {
        std::vector<double> re(mm * K);
        for (size_t e = 0; e < mm * K; ++e) re[e] = hs_pot[2 * e];
        return afq_set_system_generic(h, M, K, na, nb, re.data(), rchol, H1, ecore);
    }
    int rc = set_dims(h, AFQ_SYS_GENERIC, M, K, na, nb);
    if (rc) return rc;
    h->ecore = ecore;
    auto at = [&](int p, int q, int n, int c) { return hs_pot[2 * (((size_t)p * M + q) * K + n) + c]; };
    bool herm = true;                    // bitwise, as the symmetry test of the real entry point
    for (int p = 0; p < M && herm; ++p)
        for (int q = p; q < M && herm; ++q)
            for (int n = 0; n < K; ++n)
                if (at(p, q, n, 0) != at(q, p, n, 0) || at(p, q, n, 1) != -at(q, p, n, 1)) { herm = false; break; }
    h->hs_sym = false;
    h->hs_cplx = herm ? AFQ_HS_HERMITIAN : AFQ_HS_GENERAL;
    if (herm) {
        // Re L_n symmetric: columns p <= q (the layout of the real packed path); Im L_n antisymmetric: columns p < q
        const size_t np = (size_t)M * (M + 1) / 2, nu = (size_t)M * (M - 1) / 2;
        h->ld_hs = (long)((np + 1) & ~(size_t)1);
        h->ld_hs_im = (long)((nu + 1) & ~(size_t)1);
        std::vector<double> tr((size_t)K * h->ld_hs, 0.0), ti((size_t)K * h->ld_hs_im, 0.0);
        std::vector<int> pq(2 * np), pqi(2 * (nu ? nu : 1));
        size_t c = 0, ci = 0;
        for (int p = 0; p < M; ++p)
            for (int q = p; q < M; ++q, ++c) {
                pq[2 * c] = p; pq[2 * c + 1] = q;
                for (int n = 0; n < K; ++n) tr[(size_t)n * h->ld_hs + c] = at(p, q, n, 0);
                if (q == p) continue;
                pqi[2 * ci] = p; pqi[2 * ci + 1] = q;
                for (int n = 0; n < K; ++n) ti[(size_t)n * h->ld_hs_im + ci] = at(p, q, n, 1);
                ++ci;
            }
        if ((rc = dev_upload(h, LT_SYSTEM, &h->hs_pot, tr.data(), tr.size()))) return rc;
        if ((rc = dev_upload(h, LT_SYSTEM, &h->hs_pot_im, ti.data(), ti.size()))) return rc;
        if ((rc = dev_upload(h, LT_SYSTEM, &h->hs_pair, pq.data(), np))) return rc;
        if (nu && (rc = dev_upload(h, LT_SYSTEM, &h->hs_pair_im, pqi.data(), nu))) return rc;
    } else {
        h->ld_hs = h->ld_hs_im = (long)((mm + 1) & ~(size_t)1);
        std::vector<double> tr((size_t)K * h->ld_hs, 0.0), ti((size_t)K * h->ld_hs, 0.0);
        for (size_t r = 0; r < mm; ++r)
            for (int n = 0; n < K; ++n) {
                tr[(size_t)n * h->ld_hs + r] = hs_pot[2 * (r * K + n)];
                ti[(size_t)n * h->ld_hs + r] = hs_pot[2 * (r * K + n) + 1];
            }
        if ((rc = dev_upload(h, LT_SYSTEM, &h->hs_pot, tr.data(), tr.size()))) return rc;
        if ((rc = dev_upload(h, LT_SYSTEM, &h->hs_pot_im, ti.data(), ti.size()))) return rc;
    }
    h->ld_rc = (long)((K + 1) & ~1);
    if ((rc = upload_rchol(h, rchol, rchol_is_real(rchol, nq * K)))) return rc;
    if ((rc = dev_upload(h, LT_SYSTEM, &h->H1, H1, 2 * mm))) return rc;
    cache_of(h)->H1.assign(H1, H1 + 4 * mm);
    return AFQ_OK;
}

int afq_set_system_hubbard(afq_handle *h, int M, int na, int nb, double U, const double *T) {
    drop_walk_caches(h);
    if (!h || !T) return AFQ_EINVAL;
    int rc = set_dims(h, AFQ_SYS_HUBBARD, M, M, na, nb);
    if (rc) return rc;
    h->U = U; h->ecore = 0.0;
    const size_t mm = (size_t)M * M;
    if ((rc = dev_upload(h, LT_SYSTEM, &h->H1, T, 2 * mm))) return rc;
    cache_of(h)->H1.assign(T, T + 4 * mm);
    return AFQ_OK;
}

static int csc_to_csr(afq_handle *h, int nrow, int ncol, const int64_t *cp, const int64_t *row, const double *val,
                      int64_t **rp_d, int64_t **col_d, cplx **val_d) {
    const int64_t nnz = cp[ncol];
    std::vector<int64_t> rp(nrow + 1, 0), col(nnz);
    std::vector<double> v(2 * nnz);
    for (int64_t z = 0; z < nnz; ++z) rp[row[z] + 1]++;
    for (int r = 0; r < nrow; ++r) rp[r + 1] += rp[r];
    std::vector<int64_t> fill(rp.begin(), rp.end() - 1);
    for (int c = 0; c < ncol; ++c)
        for (int64_t z = cp[c]; z < cp[c + 1]; ++z) {
            const int64_t d = fill[row[z]]++;
            col[d] = c; v[2 * d] = val[2 * z]; v[2 * d + 1] = val[2 * z + 1];
        }
    int rc;
    if ((rc = dev_upload(h, LT_SYSTEM, rp_d, rp.data(), rp.size()))) return rc;
    if ((rc = dev_upload(h, LT_SYSTEM, col_d, col.data(), col.size()))) return rc;
    return dev_upload(h, LT_SYSTEM, val_d, v.data(), (size_t)nnz);
}

int afq_set_system_ueg(afq_handle *h, int M, int nq, int na, int nb, const int64_t *iA_colptr,
                       const int64_t *iA_row, const double *iA_val, const int64_t *iB_colptr,
                       const int64_t *iB_row, const double *iB_val, const int64_t *kpq_off,
                       const int64_t *kpq_i, const int64_t *kpq_kpq, const int64_t *pmq_off,
                       const int64_t *pmq_i, const int64_t *pmq_pmq, const double *vqvec, double vol,
                       const double *H1diag, double ecore) {
    drop_walk_caches(h);
    if (!h || !iA_colptr || !iB_colptr || !kpq_off || !pmq_off || !vqvec || !H1diag) return AFQ_EINVAL;
    int rc = set_dims(h, AFQ_SYS_UEG, M, 2 * nq, na, nb);
    if (rc) return rc;
    h->nq = nq; h->vol = vol; h->ecore = ecore;
    h->nnzA = iA_colptr[nq]; h->nnzB = iB_colptr[nq];
    if ((rc = dev_upload(h, LT_SYSTEM, &h->iA_colptr, iA_colptr, (size_t)nq + 1))) return rc;
    if ((rc = dev_upload(h, LT_SYSTEM, &h->iA_row, iA_row, (size_t)h->nnzA))) return rc;
    if ((rc = dev_upload(h, LT_SYSTEM, &h->iA_val, iA_val, (size_t)h->nnzA))) return rc;
    if ((rc = dev_upload(h, LT_SYSTEM, &h->iB_colptr, iB_colptr, (size_t)nq + 1))) return rc;
    if ((rc = dev_upload(h, LT_SYSTEM, &h->iB_row, iB_row, (size_t)h->nnzB))) return rc;
    if ((rc = dev_upload(h, LT_SYSTEM, &h->iB_val, iB_val, (size_t)h->nnzB))) return rc;
    if ((rc = csc_to_csr(h, M * M, nq, iA_colptr, iA_row, iA_val, &h->iA_rowptr, &h->iA_col, &h->iA_rval))) return rc;
    if ((rc = csc_to_csr(h, M * M, nq, iB_colptr, iB_row, iB_val, &h->iB_rowptr, &h->iB_col, &h->iB_rval))) return rc;
    {   // column-ELL layout of [iA | iB]: adjacent columns (= adjacent threads) read adjacent entries
        int L = 0;
        for (int q = 0; q < nq; ++q) {
            L = std::max(L, (int)(iA_colptr[q + 1] - iA_colptr[q]));
            L = std::max(L, (int)(iB_colptr[q + 1] - iB_colptr[q]));
        }
        const size_t nc = (size_t)2 * nq;
        std::vector<int> er(nc * L, 0);
        std::vector<double> ev(2 * nc * L, 0.0);
        for (int c = 0; c < 2 * nq; ++c) {
            const bool isB = c >= nq;
            const int q = isB ? c - nq : c;
            const int64_t *cp = isB ? iB_colptr : iA_colptr, *rw = isB ? iB_row : iA_row;
            const double *vl = isB ? iB_val : iA_val;
            int k = 0;
            for (int64_t z = cp[q]; z < cp[q + 1]; ++z, ++k) {
                er[(size_t)k * nc + c] = (int)rw[z];
                ev[2 * ((size_t)k * nc + c)] = vl[2 * z]; ev[2 * ((size_t)k * nc + c) + 1] = vl[2 * z + 1];
            }
        }
        h->ell_len = L;
        if ((rc = dev_upload(h, LT_SYSTEM, &h->ell_row, er.data(), nc * L))) return rc;
        if ((rc = dev_upload(h, LT_SYSTEM, &h->ell_val, ev.data(), nc * L))) return rc;
    }
    if ((rc = dev_upload(h, LT_SYSTEM, &h->kpq_off, kpq_off, (size_t)nq + 1))) return rc;
    if ((rc = dev_upload(h, LT_SYSTEM, &h->kpq_i, kpq_i, (size_t)kpq_off[nq]))) return rc;
    if ((rc = dev_upload(h, LT_SYSTEM, &h->kpq_kpq, kpq_kpq, (size_t)kpq_off[nq]))) return rc;
    if ((rc = dev_upload(h, LT_SYSTEM, &h->pmq_off, pmq_off, (size_t)nq + 1))) return rc;
    if ((rc = dev_upload(h, LT_SYSTEM, &h->pmq_i, pmq_i, (size_t)pmq_off[nq]))) return rc;
    if ((rc = dev_upload(h, LT_SYSTEM, &h->pmq_pmq, pmq_pmq, (size_t)pmq_off[nq]))) return rc;
    {   // rows of G referenced by the energy's index lists (estimators/ueg.py:27-88)
        std::vector<int> rmap(M, -1), rows;
        for (int64_t z = 0; z < kpq_off[nq]; ++z) if (rmap[kpq_i[z]] < 0) { rmap[kpq_i[z]] = 1; }
        for (int64_t z = 0; z < pmq_off[nq]; ++z) if (rmap[pmq_i[z]] < 0) { rmap[pmq_i[z]] = 1; }
        for (int i = 0; i < M; ++i) if (rmap[i] > 0) { rmap[i] = (int)rows.size(); rows.push_back(i); }
        h->ueg_nrows = (int)rows.size();
        if ((rc = dev_upload(h, LT_SYSTEM, &h->ueg_rmap, rmap.data(), (size_t)M))) return rc;
        if ((rc = dev_upload(h, LT_SYSTEM, &h->ueg_rows, rows.data(), rows.size()))) return rc;
        // packed copies for energy_ueg_q_kernel (M and the staged row count fit 16 bits, the list lengths 31)
        if (M < 65536 && kpq_off[nq] < (1LL << 31) && pmq_off[nq] < (1LL << 31)) {
            std::vector<int> kp((size_t)kpq_off[nq]), pm((size_t)pmq_off[nq]), ko((size_t)nq + 1), po((size_t)nq + 1);
            for (int64_t z = 0; z < kpq_off[nq]; ++z) kp[z] = (rmap[kpq_i[z]] << 16) | (int)kpq_kpq[z];
            for (int64_t z = 0; z < pmq_off[nq]; ++z) pm[z] = (rmap[pmq_i[z]] << 16) | (int)pmq_pmq[z];
            for (int q = 0; q <= nq; ++q) { ko[q] = (int)kpq_off[q]; po[q] = (int)pmq_off[q]; }
            if ((rc = dev_upload(h, LT_SYSTEM, &h->ueg_kp, kp.data(), kp.size() ? kp.size() : 1))) return rc;
            if ((rc = dev_upload(h, LT_SYSTEM, &h->ueg_pm, pm.data(), pm.size() ? pm.size() : 1))) return rc;
            if ((rc = dev_upload(h, LT_SYSTEM, &h->ueg_koff, ko.data(), ko.size()))) return rc;
            if ((rc = dev_upload(h, LT_SYSTEM, &h->ueg_poff, po.data(), po.size()))) return rc;
            // the same lists for gathers from G itself, and the deal of the pair sums on general Green's functions
            // (k_ueg_sf.hip): momentum transfers by decreasing nk * np, ties by q; those above 64 pairs take a wave each
            for (int64_t z = 0; z < kpq_off[nq]; ++z) kp[z] = ((int)kpq_i[z] << 16) | (int)kpq_kpq[z];
            for (int64_t z = 0; z < pmq_off[nq]; ++z) pm[z] = ((int)pmq_i[z] << 16) | (int)pmq_pmq[z];
            std::vector<int> order((size_t)nq);
            std::vector<long> cost((size_t)nq);
            for (int q = 0; q < nq; ++q) { order[q] = q; cost[q] = (long)(ko[q + 1] - ko[q]) * (po[q + 1] - po[q]); }
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
            h->sf_nlong = 0;
            while (h->sf_nlong < nq && cost[order[h->sf_nlong]] > 64) ++h->sf_nlong;
            if ((rc = dev_upload(h, LT_SYSTEM, &h->sf_kp, kp.data(), kp.size() ? kp.size() : 1))) return rc;
            if ((rc = dev_upload(h, LT_SYSTEM, &h->sf_pm, pm.data(), pm.size() ? pm.size() : 1))) return rc;
            if ((rc = dev_upload(h, LT_SYSTEM, &h->sf_order, order.data(), order.size() ? order.size() : 1))) return rc;
        }
    }
    if ((rc = dev_upload(h, LT_SYSTEM, &h->vqvec, vqvec, (size_t)nq))) return rc;
    if ((rc = dev_upload(h, LT_SYSTEM, &h->H1diag, H1diag, (size_t)2 * M))) return rc;
    cache_of(h)->H1.clear();
    return k_ueg_fast_system(h, M, nq, iA_colptr, iA_row, iA_val, iB_colptr, iB_row, iB_val);
}

int afq_set_trial(afq_handle *h, const double *psi) {
    drop_walk_caches(h);
    if (!h || !psi) return AFQ_EINVAL;
    if (!h->kind) AFQ_FAIL(h, AFQ_ESTATE, "set the system before the trial");
    if (h->ndet > 1) AFQ_FAIL(h, AFQ_ESTATE, "a multi-determinant trial is set; set the system again first");
    hipSetDevice(h->device);
    int rc = upload_psi(h, psi);
    if (rc) return rc;
    h->have_trial = true;
    if (h->kind == AFQ_SYS_UEG && (rc = k_ueg_fast_trial(h, psi))) return rc;
    return maybe_build_rH1(h);
}

int afq_set_trial_multi(afq_handle *h, int ndet, const double *psi, const double *coeffs, const double *rchol) {
    drop_walk_caches(h);
    if (!h || !psi || !coeffs || !rchol || ndet < 1) return AFQ_EINVAL;
    if (h->kind != AFQ_SYS_GENERIC) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "multi-determinant trials need a generic system");
    if (h->nw) AFQ_FAIL(h, AFQ_ESTATE, "set the trial before allocating walkers");
    hipSetDevice(h->device);
    free_dets(h);           // the operands afq_set_system_generic uploaded for a single determinant included
    const size_t npsi = (size_t)h->M * h->nt, nrc = npsi * h->K;
    const bool real = rchol_is_real(rchol, nrc * ndet);
    h->ndet = ndet;
    h->dets.assign(ndet, afq_handle::DetOps());
    int rc;
    for (int d = 0; d < ndet; ++d) {
        select_det(h, d, true);
        if ((rc = upload_psi(h, psi + 2 * npsi * d))) return rc;
        if ((rc = upload_rchol(h, rchol + 2 * nrc * d, real))) return rc;
        h->have_trial = true;
        if ((rc = maybe_build_rH1(h))) return rc;
    }
    select_det(h, 0);
    if ((rc = dev_upload(h, LT_TRIAL, &h->coeffs, coeffs, (size_t)ndet))) return rc;
    if (ndet > 1) {
        // conj(psi_d)^T of every determinant stacked, [ndet nt, M]: both operands of the averaged Green's function
        // (k_force_bias_msd_gbar) read it along the orbital index
        const int M = h->M, nt = h->nt;
        const size_t kkp = ((size_t)ndet * nt + 7) & ~(size_t)7;               // zero rows up to a whole chunk of 8
        std::vector<double> pt(2 * kkp * M, 0.0);
        for (int d = 0; d < ndet; ++d)
            for (int p_ = 0; p_ < M; ++p_)
                for (int i = 0; i < nt; ++i) {
                    const double *src = psi + 2 * (npsi * d + (size_t)p_ * nt + i);
                    double *dst = &pt[2 * (((size_t)d * nt + i) * M + p_)];
                    dst[0] = src[0]; dst[1] = -src[1];
                }
        if ((rc = dev_upload(h, LT_TRIAL, &h->msd_psicT, pt.data(), kkp * M))) return rc;
        if (h->hs_cplx == AFQ_HS_HERMITIAN) {
            for (double &v : pt) v = -v;
            if ((rc = dev_upload(h, LT_TRIAL, &h->msd_psicT_neg, pt.data(), kkp * M))) return rc;
        }
    }
    return AFQ_OK;
}

int afq_set_propagator(afq_handle *h, const double *BH1, const double *mf_shift, double dt, int exp_order,
                       int flags) {
    drop_walk_caches(h);
    if (!h || !BH1 || !mf_shift || dt <= 0 || exp_order < 0) return AFQ_EINVAL;
    if (!h->kind) AFQ_FAIL(h, AFQ_ESTATE, "set the system before the propagator");
    hipSetDevice(h->device);
    int rc;
    if ((rc = dev_upload(h, LT_HANDLE, &h->BH1, BH1, (size_t)2 * h->M * h->M))) return rc;
    h->bh1_real = true;
    h->bh1_same = memcmp(BH1, BH1 + (size_t)2 * h->M * h->M, sizeof(double) * 2 * h->M * h->M) == 0;
    for (size_t i = 0, n = (size_t)2 * h->M * h->M; i < n && h->bh1_real; ++i) h->bh1_real = BH1[2 * i + 1] == 0.0;
    {
        std::vector<double> &b = cache_of(h)->BH1;
        b.resize((size_t)h->M * h->M);
        for (size_t i = 0; i < b.size(); ++i) b[i] = BH1[2 * i];
    }
    if ((rc = dev_upload(h, LT_HANDLE, &h->mf_shift, mf_shift, (size_t)h->K))) return rc;
    if (h->kind == AFQ_SYS_UEG && (rc = k_ueg_fast_propagator(h, BH1))) return rc;
    h->dt = dt; h->sqrt_dt = std::pow(dt, 0.5); h->exp_order = exp_order;
    if (flags & AFQ_PROP_FREE_PROJECTION) flags &= ~AFQ_PROP_FORCE_BIAS;   // continuous.py:30-33
    const int old_nv = h->nv; const bool old_diag = h->vhs_diag;
    h->flags = flags;
    h->vhs_diag = h->kind == AFQ_SYS_HUBBARD;
    h->nv = (h->kind == AFQ_SYS_HUBBARD && (flags & AFQ_PROP_HUBBARD_SPIN)) ? 2 : 1;
    h->have_prop = true;
    if ((rc = step_operands(h))) return rc;
    if (h->nw && (old_nv != h->nv || old_diag != h->vhs_diag || !h->vhs)) {
        // (diagonal potential: a second block of the same size holds its Taylor factors)
        const size_t per = h->vhs_diag ? (size_t)2 * h->nv * h->M : (size_t)h->nv * h->M * h->M;
        if ((rc = dev_alloc(h, LT_WALKERS, &h->vhs, per * h->nw))) return rc;
    }
    return AFQ_OK;
}

// ------------------------------------------------------------------ walkers
int afq_walkers_alloc(afq_handle *h, int nw) {
    drop_walk_caches(h);
    if (!h || nw <= 0) return AFQ_EINVAL;
    if (!h->kind) AFQ_FAIL(h, AFQ_ESTATE, "set the system before allocating walkers");
    hipSetDevice(h->device);
    free_walkers(h);
    const size_t per = (size_t)h->M * h->nt, K = h->K, n = nw;
    int rc = 0;
    auto walk_as = [&](auto &slot, size_t cnt, const char *what) { return rc = dev_alloc(h, LT_WALKERS, &slot, cnt, what); };
#define walk(slot, cnt) walk_as(slot, cnt, "walkers: " #slot)
    if (walk(h->phi, per * n) || walk(h->phi_t, per * n) || walk(h->phi_t2, per * n) ||
        walk(h->weight, n) || walk(h->unscaled, n) || walk(h->detR, n) || walk(h->log_detR, n) ||
        walk(h->ot, n) || walk(h->ehyb, n) || walk(h->phase, n) || walk(h->eloc, n) ||
        walk(h->ghalf_all, per * n * h->ndet) || walk(h->ovlp_old, n) || walk(h->ovlp_new, n)) return rc;
    if (h->ndet > 1 && (walk(h->detd, n * h->ndet) || walk(h->detd_a, n * h->ndet) || walk(h->detw, n * h->ndet) ||
                        walk(h->energy_all, 3 * n * h->ndet))) return rc;
    if (walk(h->xi, K * n) || walk(h->xbar, K * n) || walk(h->xs, K * n) || walk(h->cmf, n) || walk(h->cfb, n) ||
        walk(h->energy, 3 * n) || walk(h->alive, n) || walk(h->parent_ix, n)) return rc;
    // force-bias contraction slices: enough wave-tasks to fill 1024 SIMDs
    h->fb_split = 1;
    if (h->kind == AFQ_SYS_GENERIC) {
        const long tiles = (long)((nw + 31) / 32) * ((h->K + 31) / 32) * 2;
        int sp = (int)std::max(1L, std::min(8L, 1024 / std::max(1L, tiles)));
        if (nw > 32) {
            // work-group-tiled kernel (64 walkers x 64 fields per work-group): aim at >= 512 work-groups
            const long wgt = (long)((nw + 63) / 64) * ((h->K + 63) / 64) * 2;
            sp = (int)std::max(1L, std::min(16L, (512 + wgt - 1) / wgt));
        }
        // both spins share the Cholesky block: the contraction runs once over Ghalf_a + Ghalf_b (k_force_bias_generic),
        // half as long -- measured at C3: 4 slices (8 partials for fields_kernel to add) beat 8 by 1 % of the step
        if (h->rchol_same && h->rchol_real && h->ndet == 1 && h->na == h->nb && nw > 32 && sp > 1) sp = (sp + 1) / 2;
        const int nmax = std::max(h->na, h->nb) * h->M;
        while (sp > 1 && nmax / sp < 64) --sp;
        h->fb_split = sp;
        if (walk(h->vbias_all, (size_t)2 * sp * n * K * h->ndet)) return rc;
    } else if (h->kind == AFQ_SYS_UEG) {
        if (walk(h->vbias_all, n * K) || walk(h->G, (size_t)2 * h->M * h->M * n)) return rc;
    }
    {
        // Hubbard: diagonals of up to two HS matrices, and their Taylor factors behind them
        const size_t pv = h->kind == AFQ_SYS_HUBBARD ? (size_t)4 * h->M : (size_t)h->M * h->M;
        if (walk(h->vhs, pv * n)) return rc;
    }
#undef walk
    if ((rc = dev_alloc(h, LT_WALKERS, (char **)&h->pack_tmp, std::max((size_t)nw * 2 * sizeof(int), (size_t)4096), "walkers: h->pack_tmp"))) return rc;
    h->nw = nw;
    select_det(h, h->cur_det, true);              // ghalf / vbias: the selected determinant's slices
    h->cap_frac = 0.0; h->cap_total = -1.0;       // a cap armed for an earlier population does not carry over
    {   // walker.total_weight starts as the population size (walkers/handler.py:164); with a communicator
        // the population is nw walkers on every rank
        double sc0[AFQ_NSCAL] = {0};
        sc0[0] = (double)nw * k_comm_size(h);
        AFQ_HIP(h, hipMemcpy(h->scal, sc0, sizeof(sc0), hipMemcpyHostToDevice));
    }
    // defaults of walkers/walker.py:24-61
    std::vector<double> one(nw, 1.0), zero2(2 * (size_t)nw, 0.0), one2(2 * (size_t)nw, 0.0);
    for (int i = 0; i < nw; ++i) one2[2 * i] = 1.0;
    AFQ_HIP(h, hipMemcpy(h->weight, one.data(), sizeof(double) * nw, hipMemcpyHostToDevice));
    AFQ_HIP(h, hipMemcpy(h->unscaled, one.data(), sizeof(double) * nw, hipMemcpyHostToDevice));
    AFQ_HIP(h, hipMemcpy(h->detR, one.data(), sizeof(double) * nw, hipMemcpyHostToDevice));
    AFQ_HIP(h, hipMemset(h->log_detR, 0, sizeof(double) * nw));
    AFQ_HIP(h, hipMemcpy(h->ot, one2.data(), sizeof(cplx) * nw, hipMemcpyHostToDevice));
    AFQ_HIP(h, hipMemcpy(h->phase, one2.data(), sizeof(cplx) * nw, hipMemcpyHostToDevice));
    AFQ_HIP(h, hipMemcpy(h->ehyb, zero2.data(), sizeof(cplx) * nw, hipMemcpyHostToDevice));
    AFQ_HIP(h, hipMemcpy(h->eloc, zero2.data(), sizeof(cplx) * nw, hipMemcpyHostToDevice));
    AFQ_HIP(h, hipMemset(h->phi, 0, sizeof(cplx) * per * n));
    AFQ_HIP(h, hipMemset(h->ghalf, 0, sizeof(cplx) * per * n));
    AFQ_HIP(h, hipMemset(h->energy, 0, sizeof(cplx) * 3 * n));
    AFQ_HIP(h, hipMemset(h->xi, 0, sizeof(double) * K * n));
    // fields_kernel writes the force bias, the shifted fields and their constant factors of the walkers it propagates only: a
    // walker that is dead from the start reads back zeros (AFQ_F_XBAR, AFQ_F_XSHIFTED), and the HS potential of its slot is
    // built from zeros, not from whatever the allocation held
    AFQ_HIP(h, hipMemset(h->xbar, 0, sizeof(cplx) * K * n));
    AFQ_HIP(h, hipMemset(h->xs, 0, sizeof(cplx) * K * n));
    AFQ_HIP(h, hipMemset(h->cmf, 0, sizeof(cplx) * n));
    AFQ_HIP(h, hipMemset(h->cfb, 0, sizeof(cplx) * n));
    return AFQ_OK;
}

static int field_info(afq_handle *h, int field, void **base, size_t *bytes) {
    const size_t per = (size_t)h->M * h->nt;
    switch (field) {
    case AFQ_F_PHI: *base = h->phi; *bytes = per * sizeof(cplx); break;
    case AFQ_F_WEIGHT: *base = h->weight; *bytes = sizeof(double); break;
    case AFQ_F_UNSCALED_WEIGHT: *base = h->unscaled; *bytes = sizeof(double); break;
    case AFQ_F_OT: *base = h->ot; *bytes = sizeof(cplx); break;
    case AFQ_F_HYBRID_ENERGY: *base = h->ehyb; *bytes = sizeof(cplx); break;
    case AFQ_F_PHASE: *base = h->phase; *bytes = sizeof(cplx); break;
    case AFQ_F_DETR: *base = h->detR; *bytes = sizeof(double); break;
    case AFQ_F_ELOC: *base = h->eloc; *bytes = sizeof(cplx); break;
    case AFQ_F_GHALF: *base = h->ghalf; *bytes = per * sizeof(cplx); break;
    case AFQ_F_G: *base = h->G; *bytes = (size_t)2 * h->M * h->M * sizeof(cplx); break;
    case AFQ_F_XBAR: *base = h->xbar; *bytes = (size_t)h->K * sizeof(cplx); break;
    case AFQ_F_XSHIFTED: *base = h->xs; *bytes = (size_t)h->K * sizeof(cplx); break;
    case AFQ_F_ENERGY: *base = h->energy; *bytes = 3 * sizeof(cplx); break;
    case AFQ_F_LOG_DETR: *base = h->log_detR; *bytes = sizeof(double); break;
    case AFQ_F_THERMAL_G:
        if (th_complex(h)) { *base = h->thc_G; *bytes = (size_t)2 * h->M * h->M * sizeof(cplx); break; }
        *base = h->th_G; *bytes = (size_t)2 * h->M * h->M * sizeof(double); break;
    case AFQ_F_THERMAL_STACK:
        if (th_complex(h)) { *base = h->thc_stack; *bytes = (size_t)2 * h->M * h->M * h->th_nbins * sizeof(cplx); break; }
        *base = h->th_stack; *bytes = (size_t)2 * h->M * h->M * h->th_nbins * sizeof(double); break;
    case AFQ_F_THERMAL_RIGHT: *base = th_complex(h) ? h->thc_right : nullptr; *bytes = (size_t)2 * h->M * h->M * sizeof(cplx); break;
    case AFQ_F_THERMAL_M0: *base = th_complex(h) ? h->thc_M0 : nullptr; *bytes = 2 * sizeof(cplx); break;
    case AFQ_F_THERMAL_DET: *base = th_complex(h) ? h->thc_det : nullptr; *bytes = 2 * sizeof(cplx); break;
    case AFQ_F_CMF: *base = h->cmf; *bytes = sizeof(cplx); break;
    case AFQ_F_CFB: *base = h->cfb; *bytes = sizeof(cplx); break;
    default: AFQ_FAIL(h, AFQ_EINVAL, "unknown walker field");
    }
    if (!*base) AFQ_FAIL(h, AFQ_ESTATE, "walker field not allocated (afq_walkers_alloc / afq_greens first)");
    return AFQ_OK;
}

static int ensure_spin_ghalf(afq_handle *h);

int afq_walkers_set(afq_handle *h, int field, const void *host, int first, int count) {
    if (h && (field == AFQ_F_PHI || field == AFQ_F_GHALF)) { h->gf.drop(); h->gf.rewritten(); }
    if (h && field == AFQ_F_PHI) h->step.handover.drop();
    if (!h || !host) return AFQ_EINVAL;
    if (!h->nw) AFQ_FAIL(h, AFQ_ESTATE, "no walkers allocated");
    if (first < 0 || count < 0 || first + count > h->nw) AFQ_FAIL(h, AFQ_EINVAL, "walker range out of bounds");
    if (field == AFQ_F_THERMAL_DET || field == AFQ_F_CMF || field == AFQ_F_CFB)
        AFQ_FAIL(h, AFQ_EINVAL, "afq_walkers_set: a result of the last kernel, not walker state (get only)");
    hipSetDevice(h->device);
    void *base; size_t bytes;
    int rc = field_info(h, field, &base, &bytes);
    if (rc) return rc;
    AFQ_HIP(h, hipMemcpyAsync((char *)base + bytes * first, host, bytes * count, hipMemcpyHostToDevice, h->stream));
    AFQ_HIP(h, hipStreamSynchronize(h->stream));
    return AFQ_OK;
}

int afq_walkers_get(afq_handle *h, int field, void *host, int first, int count) {
    if (!h || !host) return AFQ_EINVAL;
    if (!h->nw) AFQ_FAIL(h, AFQ_ESTATE, "no walkers allocated");
    if (first < 0 || count < 0 || first + count > h->nw) AFQ_FAIL(h, AFQ_EINVAL, "walker range out of bounds");
    hipSetDevice(h->device);
    void *base; size_t bytes;
    int rc = field_info(h, field, &base, &bytes);
    if (rc) return rc;
    if (field == AFQ_F_GHALF && (rc = ensure_spin_ghalf(h))) return rc;
    AFQ_HIP(h, hipMemcpyAsync(host, (char *)base + bytes * first, bytes * count, hipMemcpyDeviceToHost, h->stream));
    AFQ_HIP(h, hipStreamSynchronize(h->stream));
    return AFQ_OK;
}

int afq_walkers_device_ptr(afq_handle *h, int field, void **dev_ptr, int64_t *bytes_per_walker) {
    if (!h || !dev_ptr) return AFQ_EINVAL;
    void *base; size_t bytes;
    int rc = field_info(h, field, &base, &bytes);
    if (rc) return rc;
    // a reader of the per-spin Ghalf must find the CURRENT walkers' there: a step announced with afq_estimates_fuse_next
    // leaves only overlap + spin sum behind
    if (field == AFQ_F_GHALF && h->gf.kept == GreensCache::SUM_ONLY) {
        hipSetDevice(h->device);
        if ((rc = ensure_spin_ghalf(h))) return rc;
    }
    h->gf.drop(); h->gf.enabled = false;                 // the caller may write through the pointer
    if (field == AFQ_F_PHI) { h->step.handover.drop(); h->step.handover.enabled = false; }
    *dev_ptr = base;
    if (bytes_per_walker) *bytes_per_walker = (int64_t)bytes;
    return AFQ_OK;
}

// ----------------------------------------------------------------- hot path
static int greens_any(afq_handle *h, cplx *det_out, bool with_ghalf, GreensRequest req = GreensRequest(),
                      GreensResult *res = nullptr);

// The last step left its Green's function behind as overlap + spin sum of Ghalf only (afq_propagate_finish on a step the
// driver announced with afq_estimates_fuse_next): somebody wants the per-spin Ghalf after all -- evaluate it.
static int ensure_spin_ghalf(afq_handle *h) {
    if (h->gf.kept != GreensCache::SUM_ONLY) return AFQ_OK;
    h->gf.drop();
    const int rc = greens_any(h, h->ovlp_new, true);
    if (rc == AFQ_OK) h->gf.keep(GreensCache::FULL);
    return rc;
}

int afq_greens(afq_handle *h, int want_G, double *ovlp_out) {
    AFQ_API(h, "afq_greens");
    if (h) h->gf.drop();
    if (!h) return AFQ_EINVAL;
    int rc = need_ready(h, false);
    if (rc) return rc;
    {
        PhaseTimer t(h, T_GREENS);
        if ((rc = greens_any(h, h->ovlp_old, true))) return rc;
        if (want_G || h->kind == AFQ_SYS_UEG) {
            if ((rc = ensure_G(h))) return rc;
            if ((rc = k_full_G(h))) return rc;
        }
    }
    return copy_out(h, ovlp_out, h->ovlp_old, sizeof(cplx) * h->nw);
}

int afq_inverse_overlap(afq_handle *h, double *oinv_out, double *ovlp_out) {
    if (h) h->gf.drop();
    if (!h || !oinv_out) return AFQ_EINVAL;
    int rc = need_ready(h, false);
    if (rc) return rc;
    if (h->ndet > 1) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "inverse overlaps: single-determinant trials");
    const size_t nmax = h->na > h->nb ? h->na : h->nb, n = (size_t)h->nw * 2 * nmax * nmax;
    DevTemp<cplx> tmp;
    if ((rc = dev_temp(h, tmp, n))) return rc;
    AFQ_HIP(h, hipMemsetAsync(tmp, 0, sizeof(cplx) * n, h->stream));
    if ((rc = k_alive(h))) return rc;
    // every walker, dead or alive: flag them all for this call
    std::vector<int> ones(h->nw, 1);
    AFQ_HIP(h, hipMemcpyAsync(h->alive, ones.data(), sizeof(int) * h->nw, hipMemcpyHostToDevice, h->stream));
    rc = k_inverse_overlap(h, tmp, h->ovlp_new);
    if (!rc) rc = copy_out(h, oinv_out, tmp, sizeof(cplx) * n);
    if (!rc && ovlp_out) rc = copy_out(h, ovlp_out, h->ovlp_new, sizeof(cplx) * h->nw);
    if (!rc) rc = k_alive(h);
    return rc;
}

int afq_calc_overlap(afq_handle *h, double *ovlp_out) {
    AFQ_API(h, "afq_calc_overlap");
    if (h) h->gf.drop();
    if (!h) return AFQ_EINVAL;
    int rc = need_ready(h, false);
    if (rc) return rc;
    {
        PhaseTimer t(h, T_OVLP);
        if ((rc = greens_any(h, h->ovlp_new, false))) return rc;
    }
    return copy_out(h, ovlp_out, h->ovlp_new, sizeof(cplx) * h->nw);
}

// force bias from the current Ghalf / G -> h->xbar (unclipped)
// Green's function (with_ghalf) or overlap only, for every determinant of the trial.  Multi-determinant:
// per-determinant Ghalf_d / <D_d|phi> into the slices, then weights conj(c_d) <D_d|phi> and their sum
// (walkers/multi_det.py:194-229 and :135-162).
static int greens_any(afq_handle *h, cplx *det_out, bool with_ghalf, GreensRequest req, GreensResult *res) {
    int rc;
    if (h->ndet <= 1) return with_ghalf ? k_greens(h, det_out, req, res) : k_overlap(h, det_out, req, res);
    for (int d = 0; d < h->ndet; ++d) {
        select_det(h, d);
        cplx *dd = h->detd + (size_t)d * h->nw;
        req.det_a = with_ghalf ? h->detd_a + (size_t)d * h->nw : nullptr;
        rc = with_ghalf ? k_greens(h, dd, req, res) : k_overlap(h, dd, req, res);
        if (rc) { select_det(h, 0); return rc; }
    }
    select_det(h, 0);
    return k_msd_combine(h, det_out, with_ghalf);       // (multi_det.py:209,218 skip; calc_overlap :135-162 does not)
}

static int force_bias(afq_handle *h, bool with_xbar = true) {
    int rc;
    if (h->flags & AFQ_PROP_FORCE_BIAS) {
        if (h->kind == AFQ_SYS_GENERIC) {
            h->msd_fb_gbar = false;
            // (automatic mode: when every determinant's own contraction is current -- the Coulomb vectors of the energy
            //  evaluation that has just run on these Green's functions -- their weighted average costs nothing)
            if (k_msd_gbar_wanted(h) && !(h->msd_fb_mode == 0 && k_msd_vbias_current(h))) {
                // the reference's own formulation: ONE contraction with the determinant-averaged G (generic.py:154-157)
                if ((rc = k_force_bias_msd_gbar(h))) return rc;
                h->msd_fb_gbar = true;
            } else {
                for (int d = 0; d < h->ndet; ++d) {
                    select_det(h, d);
                    if ((rc = k_force_bias_generic(h))) { select_det(h, 0); return rc; }
                }
                select_det(h, 0);
            }
        }
        else if (h->kind == AFQ_SYS_UEG) { if ((rc = k_vbias_ueg(h))) return rc; }
    }
    return with_xbar ? k_xbar(h) : AFQ_OK;
}

static int local_energy(afq_handle *h);
static int local_energy_dets(afq_handle *h);

int afq_propagate(afq_handle *h, const double *xi, double eshift_re, double eshift_im) {
    if (h) { h->step.one_call = true; h->step.eshift = cmake(eshift_re, eshift_im); }
    const int rc = afq_propagate_begin(h, xi);
    if (h) h->step.one_call = false;
    if (rc && h) h->step.tail_done = false;
    return rc ? rc : afq_propagate_finish(h, eshift_re, eshift_im);
}

int afq_propagate_begin(afq_handle *h, const double *xi) {
    AFQ_API(h, "afq_propagate");
    if (!h) return AFQ_EINVAL;
    int rc = need_ready(h, true);
    if (rc) return rc;
    if (h->hirsch) AFQ_FAIL(h, AFQ_ESTATE, "discrete Hirsch propagator set: use afq_propagate_hirsch");
    // Hubbard, continuous fields, one field per site: fields_kernel makes the fields (and draws them), the diagonal HS
    // potential and its Taylor factors.  ONE flag decides the inline draw, the branch below and who writes the factors.
    const bool hubbard_fused = h->vhs_diag;
    const bool hubbard_fused_fields = hubbard_fused && h->K == h->M;
    if (xi) {
        if ((rc = k_alive(h))) return rc;
        AFQ_HIP(h, hipMemcpyAsync(h->xi, xi, sizeof(double) * (size_t)h->nw * h->K, hipMemcpyHostToDevice, h->stream));
    } else if (k_prop_fused_supported(h) || k_ueg_fast_supported(h) || hubbard_fused_fields) {
        // nothing ahead of fields_kernel reads the fields or the alive flags on this path (the Green's function is
        // evaluated for every walker, the one-body product sits inside the fused propagator): fields_kernel draws
        // the same Philox stream itself and sets the flags
        h->rng_inline = true;
        h->rng_inline_counter = h->rng_counter++;
    } else {
        if ((rc = k_rng_normal(h))) return rc;           // draws the fields and sets the alive flags
    }
    const bool fp = (h->flags & AFQ_PROP_FREE_PROJECTION) != 0;
    if (!fp || (h->flags & AFQ_PROP_FORCE_BIAS)) {
        PhaseTimer t(h, T_GREENS);                         // continuous.py:245
        // (the spin sum alone will not do when this step needs more than the force bias: local-energy weights, one_rdm)
        const GreensCache::Kept kept = h->gf.kept;
        const bool sum_ok = kept == GreensCache::SUM_ONLY && (h->flags & AFQ_PROP_HYBRID) && !h->rdm_on &&
                            (h->kind == AFQ_SYS_GENERIC ||
                             (h->kind == AFQ_SYS_HUBBARD && h->gdiag && h->gf.gdiag.current(h->gf)));
        if (kept == GreensCache::FULL || sum_ok) std::swap(h->ovlp_old, h->ovlp_new);   // computed at the end of the last step
                                                     // (SUM_ONLY: as overlap + spin sum of Ghalf, all the force bias reads)
        else if ((rc = greens_any(h, h->ovlp_old, true))) return rc;
        h->gf.drop();                                      // (the step rewrites phi)
        const bool le = !fp && !(h->flags & AFQ_PROP_HYBRID);
        // (the plane-wave fast step gathers the force bias from the occupied rows of G built from Ghalf: no full G)
        if ((h->kind == AFQ_SYS_UEG && ((h->flags & AFQ_PROP_FORCE_BIAS) || le) && !k_ueg_fast_supported(h)) ||
            (h->rdm_on && h->ndet == 1)) {
            // (one_rdm: walker.G = the Green's function of the walker before this step, continuous.py:245)
            if ((rc = ensure_G(h))) return rc;
            if ((rc = k_full_G(h))) return rc;
        }
        if (le) {
            // walker.local_energy(system) of the un-propagated walker (continuous.py:296)
            PhaseTimer te(h, T_ENERGY);
            // Multi-determinant: the reference combines the per-determinant energies of the UN-propagated
            // walker with the weights calc_overlap refreshes for the PROPAGATED walker
            // (continuous.py:296 after :261, multi_det.py:160), so only the per-determinant part runs here.
            if (h->ndet > 1) { if ((rc = local_energy_dets(h))) return rc; }
            else if ((rc = local_energy(h))) return rc;
        }
    }
    if (k_ueg_fast_supported(h) || hubbard_fused || !k_prop_fused_supported(h)) h->step.handover.drop();   // (not the fused propagator)
    if (k_ueg_fast_supported(h)) {
        // plane waves: force bias from the occupied rows of G, fields, and the ~2 nq coefficients that ARE the HS
        // potential, in one launch; B exp(V) B from those coefficients in a second one (k_ueg.hip)
        // (one launch -- ueg_step_kernel -- when the propagator's LDS arrays fit behind the field part's, else two)
        { PhaseTimer t(h, T_EXP); if ((rc = k_ueg_step(h))) return rc; }                         // :133-171, :251, :258
        h->prop_pending = true;
        return AFQ_OK;
    }
    if (hubbard_fused) {
        // Hubbard, continuous fields: the HS potential is diagonal, exp(V) a row scaling.  The force bias reads Ghalf of
        // the un-propagated walker, so fields, potential and the scaling factors are made FIRST and the factors ride on
        // the store of the first one-body product: phi <- B [exp(V) (B phi)] in two GEMM launches, the walkers pass
        // through memory twice instead of three times (exp_diag_kernel: 537 MB of traffic at C4).
        cplx *fac = h->vhs + (size_t)h->nw * h->nv * h->M;                              // second half of the vhs buffer
        const bool fields_make_factors = hubbard_fused_fields;                          // (one field per site)
        {
            PhaseTimer t(h, T_FB);                                                      // :133-158
            if ((rc = force_bias(h, false))) return rc;
            // ... and with the fields the diagonal HS potential (:161) and its Taylor factors (:162-171): the same
            // arithmetic as vhs_hubbard_kernel + exp_diag_factor_kernel, two launches less
            if ((rc = k_xbar_fields(h, fields_make_factors ? fac : nullptr))) return rc;
        }
        if (!fields_make_factors) {
            { PhaseTimer t(h, T_VHS); if ((rc = build_vhs(h))) return rc; }             // :161
            { PhaseTimer t(h, T_EXP); if ((rc = k_exp_diag_factors(h, h->vhs, fac))) return rc; }   // :162-171
        }
        if (h->rng_inline) AFQ_FAIL(h, AFQ_ESTATE, "internal: the inline field draw of this step was not consumed by the field kernel");
        { PhaseTimer t(h, T_ONEBODY); if ((rc = k_onebody(h, fac))) return rc; }        // :251 + the row scaling
        { PhaseTimer t(h, T_ONEBODY); if ((rc = k_onebody(h))) return rc; }             // :258
        h->prop_pending = true;
        return AFQ_OK;
    }
    // The force bias reads Ghalf of the un-propagated walker, so building the HS potential commutes
    // with the first one-body product; the fused path uses that to run B exp(V) B in one launch.
    const bool fused = k_prop_fused_supported(h);
    // Large systems (the GEMM chain): one matrix serves both spins and the HS potential never depends on the spin, so a walker
    // whose spin blocks are bitwise equal -- every walker of a run that starts closed-shell -- keeps them equal through
    // B exp(V) B.  Checked on the walkers themselves at every step (closed_flags_kernel); the GEMMs then leave out the tiles of
    // the beta columns of such walkers and the alpha block is copied over the beta block behind the closing one-body product.
    h->closed_large = !fused && h->kind == AFQ_SYS_GENERIC && h->nv == 1 && h->bh1_same && h->na == h->nb && h->na > 0 &&
                      h->M > 128 && h->nt > 32 && h->nw >= 64;
    struct ClosedLargeOff { afq_handle *h; ~ClosedLargeOff() { h->closed_large = false; } } closed_large_off{h};   // on every way out
    if (h->closed_large && (rc = k_closed_flags(h))) return rc;
    if (!fused) { PhaseTimer t(h, T_ONEBODY); if ((rc = k_onebody(h))) return rc; }   // :251
    {
        PhaseTimer t(h, T_FB);                                                      // :133-158
        if ((rc = force_bias(h, false))) return rc;
        if ((rc = k_xbar_fields(h))) return rc;
    }
    // symmetric L_n and the fused propagator as the only consumer: the HS potential is stored as its upper
    // triangle only (no scattered mirror writes) and the propagator fetches V[k][row] for k < row
    h->step.vhs_upper = fused && h->hs_sym;
    { PhaseTimer t(h, T_VHS); rc = build_vhs(h); }                                  // :161
    if (rc) { h->step.vhs_upper = false; return rc; }
    if (fused && k_step_fuses(h)) {
        PhaseTimer t(h, T_EXP);                                                     // :251, :162-171, :258, :261-292
        // the closing evaluation of afq_propagate_finish, asked for here with the same request and run by the propagator's launch
        // (scope 1: without the shift -- begin alone -- the weight update stays with finish; unannounced, somebody may read
        //  the per-spin Ghalf)
        GreensRequest req;
        req.ride_weight = h->step.one_call;
        if (h->step.one_call) req.eshift = h->step.eshift;
        req.may_skip_store = h->fuse_est_req;
        h->step.tail_res = GreensResult();
        rc = k_prop_fused_greens(h, req, &h->step.tail_res, h->step.get(StepState::FUSION) == 2);
        h->step.vhs_upper = false;
        if (rc) return rc;
        h->step.tail_done = true;
    } else if (fused) {
        PhaseTimer t(h, T_EXP);                                                     // :251, :162-171, :258
        rc = k_prop_fused(h);
        h->step.vhs_upper = false;
        if (rc) return rc;
    } else {
        { PhaseTimer t(h, T_EXP); if ((rc = apply_exp(h, h->vhs))) return rc; }    // :162-171
        { PhaseTimer t(h, T_ONEBODY); if ((rc = k_onebody(h))) return rc; }        // :258
        if (h->closed_large && (rc = k_closed_copy_beta(h))) return rc;
    }
    h->prop_pending = true;
    return AFQ_OK;
}

int afq_propagate_finish(afq_handle *h, double eshift_re, double eshift_im) {
    AFQ_API(h, "afq_propagate");
    if (!h) return AFQ_EINVAL;
    if (!h->prop_pending) AFQ_FAIL(h, AFQ_ESTATE, "afq_propagate_finish without afq_propagate_begin");
    hipSetDevice(h->device);
    h->prop_pending = false;
    int rc;
    const bool fp = (h->flags & AFQ_PROP_FREE_PROJECTION) != 0;
    {
        PhaseTimer t(h, T_OVLP);                                                    // :261-262
        // The overlap of the propagated walker is the determinant of the matrix whose inverse the next
        // step's Green's function needs (continuous.py:245 of step n+1), so factorise once: this call
        // leaves Ghalf of the NEW phi behind and the next afq_propagate / afq_estimates_update reuses it.
        const bool le_msd = h->ndet > 1 && !fp && !(h->flags & AFQ_PROP_HYBRID);
        GreensRequest req;
        GreensResult res;
        req.ride_weight = h->ndet == 1 && !le_msd;          // single determinant: k_greens may take the weight update along
        req.eshift = cmake(eshift_re, eshift_im);
        if (h->step.tail_done) {
            // (the propagator's launch has evaluated it: overlap and spin sum; the per-spin store unless the step was announced
            //  ahead of it; the weight update unless begin ran without the shift -- weight_rode is false then and it runs below)
            h->step.tail_done = false;
            res = h->step.tail_res;
            h->gf.keep(res.store_skipped ? GreensCache::SUM_ONLY : GreensCache::FULL);
        } else if (h->gf.enabled && !fp) {
            // afq_estimates_fuse_next told us that nothing but the next step's force bias will read this Green's function
            // (no comb, no energy, no block end behind this step): when that force bias contracts the spin sum
            // Ghalf_a + Ghalf_b (k_fb_use_sum), the per-spin Ghalf -- 2/3 of the kernel's stores, 20 MB per step at C3 --
            // is not written at all.  Everything else sees "no cached Green's function" and recomputes if it asks.
            // (Hubbard, continuous fields, N > 45: the force bias reads the diagonal sums the Ghalf GEMM leaves behind --
            //  268 MB of Ghalf per step at C4 that nobody reads)
            const bool fb_sum = h->kind == AFQ_SYS_GENERIC && k_fb_use_sum(h);
            const bool fb_diag = h->kind == AFQ_SYS_HUBBARD && !h->hirsch && h->psicT && k_greens_big_supported(h);
            req.may_skip_store = h->fuse_est_req && h->ndet == 1 && (fb_sum || fb_diag) &&
                                 (h->flags & AFQ_PROP_HYBRID) && (h->flags & AFQ_PROP_FORCE_BIAS) && !h->rdm_on &&
                                 h->nbp == 0 && h->psi_stride == 0;
            if ((rc = greens_any(h, h->ovlp_new, true, req, &res))) return rc;
            h->gf.keep(res.store_skipped ? GreensCache::SUM_ONLY : GreensCache::FULL);
        } else if ((rc = greens_any(h, h->ovlp_new, false, req, &res))) return rc;
        if (h->ndet > 1 && !fp && !(h->flags & AFQ_PROP_HYBRID)) {
            if ((rc = k_msd_energy_combine(h))) return rc;
        }
        if (!res.weight_rode && (rc = k_update_weight(h, req.eshift))) return rc;
        if (h->nbp > 0 && !fp && (rc = k_bp_push(h))) return rc;     // FieldConfig.update (continuous.py:288-289)
    }
    if (h->fuse_est_req) {                                // afq_estimates_fuse_next: the weight update took the terms along
        h->fuse_est_req = false;
        h->est_acc_pending = true;
    }
    return AFQ_OK;
}

int afq_estimates_fuse_next(afq_handle *h) {
    if (!h) return AFQ_EINVAL;
    if (!h->nw) AFQ_FAIL(h, AFQ_ESTATE, "no walkers");
    if (h->rdm_on) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "afq_estimates_fuse_next with the one-body RDM accumulation on");
    if (h->hirsch) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "afq_estimates_fuse_next: continuous propagator only");
    hipSetDevice(h->device);
    if (!h->est_acc) {
        int rc = dev_alloc(h, LT_WALKERS, &h->est_acc, (size_t)6 * h->nw);
        if (rc) return rc;
        AFQ_HIP(h, hipMemsetAsync(h->est_acc, 0, sizeof(double) * 6 * h->nw, h->stream));
    }
    h->fuse_est_req = true;
    return AFQ_OK;
}

// use_log_shift (walkers/handler.py:45,228,456-475).  The shifts are the same for every walker (walker.py:49-52 and
// the update at handler.py:471-474), so they live on the handle; log_detR is walker state.
int afq_set_log_shift(afq_handle *h, int on, double log_shift, double detR_shift) {
    AFQ_API(h, "afq_set_log_shift");
    if (!h) return AFQ_EINVAL;
    if (on && h->ndet > 1) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "use_log_shift: single-determinant walkers only");
    h->log_shift_on = on != 0;
    h->log_shift = on ? log_shift : 0.0;
    h->detR_shift = on ? detR_shift : 0.0;
    return AFQ_OK;
}

int afq_log_ovlp_sums(afq_handle *h, double *sums3) {
    AFQ_API(h, "afq_log_ovlp_sums");
    if (!h || !sums3) return AFQ_EINVAL;
    int rc = need_ready(h, false);
    if (rc) return rc;
    return k_log_ovlp_sums(h, sums3);
}

int afq_reortho(afq_handle *h, double *detR_out) {
    AFQ_API(h, "afq_reortho");
    if (!h) return AFQ_EINVAL;
    h->step.handover.drop();            // (phi -> phi R^-1: the Green's function survives the QR, B phi does not)
    int rc = need_ready(h, false);
    if (rc) { h->gf.drop(); return rc; }
    // Ghalf = (phi^T psi*)^-1 phi^T does not change when phi -> phi R^-1, so a Green's function kept from
    // the end of the last step stays valid across the QR; only the cached overlap picks up 1 / det R.
    // (the spin sum of Ghalf is as invariant as Ghalf itself: either kept state stays)
    const GreensCache::Kept kept = h->gf.take();
    const bool keep = kept != GreensCache::NOTHING && h->ndet == 1;
    bool scaled = false;
    { PhaseTimer t(h, T_QR); if ((rc = k_reortho(h, keep ? h->ovlp_new : nullptr, &scaled))) return rc; }
    if (keep) {
        if (!scaled && (rc = k_scale_by_inverse(h, h->ovlp_new, h->detR))) return rc;
        h->gf.keep(kept);
    }
    // the cached overlap above needs det R itself; walker.detR / walker.ot / log_detR take the shifted one
    if (h->log_shift_on && (rc = k_log_shift_reortho(h))) return rc;
    return copy_out(h, detR_out, h->detR, sizeof(double) * h->nw);
}

// per-determinant energies E[G_d] from the half-rotated operands of determinant d (algebraically the
// full-G energy of estimators/generic.py:398-434 evaluated on G_d = conj(psi_d) Ghalf_d)
static int local_energy_dets(afq_handle *h) {
    cplx *final_e = h->energy;
    int rc = AFQ_OK;
    for (int d = 0; d < h->ndet && !rc; ++d) {
        select_det(h, d);
        h->energy = h->energy_all + (size_t)d * 3 * h->nw;
        rc = k_energy_generic(h);
    }
    h->energy = final_e;
    select_det(h, 0);
    return rc;
}

static int local_energy(afq_handle *h) {
    if (h->kind == AFQ_SYS_GENERIC && h->ndet > 1) {
        int rc = local_energy_dets(h);
        if (rc) return rc;
        return k_msd_energy_combine(h);              // estimators/mixed.py:439-448
    }
    if (h->kind == AFQ_SYS_GENERIC) return k_energy_generic(h);
    if (h->kind == AFQ_SYS_HUBBARD) return k_energy_hubbard(h);
    if (!h->G) AFQ_FAIL(h, AFQ_ESTATE, "afq_greens must run before afq_local_energy");
    return k_energy_ueg(h);
}

int afq_local_energy(afq_handle *h, double *E_out) {
    AFQ_API(h, "afq_local_energy");
    if (!h) return AFQ_EINVAL;
    int rc = need_ready(h, false);
    if (rc) return rc;
    if (!h->rH1 && h->kind != AFQ_SYS_UEG) AFQ_FAIL(h, AFQ_ESTATE, "half-rotated H1 missing (set trial)");
    if ((rc = ensure_spin_ghalf(h))) return rc;
    { PhaseTimer t(h, T_ENERGY); if ((rc = local_energy(h))) return rc; }
    return copy_out(h, E_out, h->energy, sizeof(cplx) * 3 * h->nw);
}

int afq_set_exchange_algorithm(afq_handle *h, int mode) {
    if (!h || mode < 0 || mode > 2) return AFQ_EINVAL;
    h->exx_mode = mode;
    return AFQ_OK;
}

// the switches of the fused step: validated, stored and the hand-over dropped by their owner (StepState::set)
static int set_step_switch(afq_handle *h, StepState::Switch which, int value) {
    return h && h->step.set(which, value) ? AFQ_OK : AFQ_EINVAL;        // (a refused value leaves the handle untouched)
}
int afq_set_propagator_closed_form(afq_handle *h, int mode) { return set_step_switch(h, StepState::CLOSED_FORM, mode); }
int afq_set_step_fusion(afq_handle *h, int mode) { return set_step_switch(h, StepState::FUSION, mode); }
int afq_set_step_fusion_scope(afq_handle *h, int scope) { return set_step_switch(h, StepState::SCOPE, scope); }
int afq_set_step_tail_overlap(afq_handle *h, int on) { return set_step_switch(h, StepState::TAIL_OVERLAP, on); }
int afq_set_step_handover(afq_handle *h, int on) { return set_step_switch(h, StepState::HANDOVER, on); }

int afq_propagator_closed_form(afq_handle *h, int *mode) {
    if (!h || !mode) return AFQ_EINVAL;
    *mode = k_prop_closed_resident(h) ? 2 : 1;
    return AFQ_OK;
}

int afq_set_msd_force_bias(afq_handle *h, int mode) {
    if (!h || mode < 0 || mode > 2) return AFQ_EINVAL;
    h->msd_fb_mode = mode;
    return AFQ_OK;
}

int afq_msd_force_bias(afq_handle *h, int *mode) {
    if (!h || !mode) return AFQ_EINVAL;
    if (h->kind != AFQ_SYS_GENERIC || !h->have_trial || !h->nw) AFQ_FAIL(h, AFQ_ESTATE, "generic system, trial and walkers must be set");
    *mode = h->ndet <= 1 ? 0 : k_msd_gbar_wanted(h) ? 2 : 1;
    return AFQ_OK;
}

int afq_exchange_algorithm(afq_handle *h, int *mode) {
    if (!h || !mode) return AFQ_EINVAL;
    if (h->kind != AFQ_SYS_GENERIC || !h->have_trial) AFQ_FAIL(h, AFQ_ESTATE, "generic system and trial must be set");
    *mode = k_exchange_uses_quadratic(h) ? 2 : 1;
    return AFQ_OK;
}

// ---------------------------------------------------------------- test hooks
int afq_force_bias(afq_handle *h, double *xbar_out) {
    if (!h) return AFQ_EINVAL;
    int rc = need_ready(h, true);
    if (rc) return rc;
    if ((rc = force_bias(h))) return rc;
    return copy_out(h, xbar_out, h->xbar, sizeof(cplx) * (size_t)h->nw * h->K);
}

int afq_shift_fields(afq_handle *h, const double *xi, const double *xbar, double *xs_out, double *cmf_out,
                     double *cfb_out) {
    if (!h || !xi || !xbar) return AFQ_EINVAL;
    int rc = need_ready(h, true);
    if (rc) return rc;
    const size_t n = (size_t)h->nw * h->K;
    AFQ_HIP(h, hipMemcpyAsync(h->xi, xi, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
    AFQ_HIP(h, hipMemcpyAsync(h->xbar, xbar, sizeof(cplx) * n, hipMemcpyHostToDevice, h->stream));
    if ((rc = k_fields_explicit(h, h->xi, h->xbar, h->xs, h->cmf, h->cfb))) return rc;
    if ((rc = copy_out(h, xs_out, h->xs, sizeof(cplx) * n))) return rc;
    if ((rc = copy_out(h, cmf_out, h->cmf, sizeof(cplx) * h->nw))) return rc;
    return copy_out(h, cfb_out, h->cfb, sizeof(cplx) * h->nw);
}

int afq_vhs_count(afq_handle *h, int *nv) {
    if (!h || !nv) return AFQ_EINVAL;
    *nv = h->nv;
    return AFQ_OK;
}

// Dense M x M matrices out, whatever the internal storage
int afq_vhs(afq_handle *h, const double *xs, double *vhs_out) {
    if (!h || !xs || !vhs_out) return AFQ_EINVAL;
    int rc = need_ready(h, true);
    if (rc) return rc;
    const size_t n = (size_t)h->nw * h->K;
    AFQ_HIP(h, hipMemcpyAsync(h->xs, xs, sizeof(cplx) * n, hipMemcpyHostToDevice, h->stream));
    if ((rc = build_vhs(h))) return rc;
    const size_t mm = (size_t)h->M * h->M;
    if (!h->vhs_diag) return copy_out(h, vhs_out, h->vhs, sizeof(cplx) * mm * h->nv * h->nw);
    std::vector<double> d((size_t)2 * h->nw * h->nv * h->M);
    if ((rc = copy_out(h, d.data(), h->vhs, sizeof(cplx) * (size_t)h->nw * h->nv * h->M))) return rc;
    std::memset(vhs_out, 0, sizeof(cplx) * mm * h->nv * h->nw);
    for (size_t b = 0; b < (size_t)h->nw * h->nv; ++b)
        for (int p = 0; p < h->M; ++p) {
            vhs_out[2 * (b * mm + (size_t)p * h->M + p)] = d[2 * (b * h->M + p)];
            vhs_out[2 * (b * mm + (size_t)p * h->M + p) + 1] = d[2 * (b * h->M + p) + 1];
        }
    return AFQ_OK;
}

int afq_apply_exponential(afq_handle *h, const double *vhs) {
    drop_walk_caches(h);
    if (!h || !vhs) return AFQ_EINVAL;
    int rc = need_ready(h, true);
    if (rc) return rc;
    if ((rc = k_alive(h))) return rc;
    const size_t mm = (size_t)h->M * h->M;
    if (!h->vhs_diag) {
        AFQ_HIP(h, hipMemcpyAsync(h->vhs, vhs, sizeof(cplx) * mm * h->nv * h->nw, hipMemcpyHostToDevice, h->stream));
    } else {
        std::vector<double> d((size_t)2 * h->nw * h->nv * h->M);
        for (size_t b = 0; b < (size_t)h->nw * h->nv; ++b)
            for (int p = 0; p < h->M; ++p) {
                d[2 * (b * h->M + p)] = vhs[2 * (b * mm + (size_t)p * h->M + p)];
                d[2 * (b * h->M + p) + 1] = vhs[2 * (b * mm + (size_t)p * h->M + p) + 1];
            }
        AFQ_HIP(h, hipMemcpy(h->vhs, d.data(), sizeof(double) * d.size(), hipMemcpyHostToDevice));
    }
    if ((rc = apply_exp(h, h->vhs))) return rc;
    return afq_sync(h);
}

int afq_kinetic(afq_handle *h) {
    drop_walk_caches(h);
    if (!h) return AFQ_EINVAL;
    int rc = need_ready(h, true);
    if (rc) return rc;
    if ((rc = k_alive(h))) return rc;
    if ((rc = k_onebody(h))) return rc;
    return afq_sync(h);
}

// -------------------------------------------------------------- driver glue
int afq_set_weight_cap(afq_handle *h, double frac, double total_weight) {
    if (!h) return AFQ_EINVAL;
    h->cap_frac = frac > 0.0 ? frac : 0.0;
    h->cap_total = total_weight;
    return AFQ_OK;
}

int afq_cap_weights(afq_handle *h, double frac, double total_weight) {
    if (!h) return AFQ_EINVAL;
    if (th_thermal(h) && h->nw) { hipSetDevice(h->device); return k_cap_weights(h, frac, total_weight); }   // (no trial determinant)
    int rc = need_ready(h, false);
    if (rc) return rc;
    return k_cap_weights(h, frac, total_weight);
}

int afq_popcontrol_comb(afq_handle *h, double r, double target_weight, int32_t *parent_ix,
                        double *total_weight_out) {
    if (h) h->scal_cache_valid = false;
    AFQ_API(h, "afq_popcontrol_comb");
    if (!h) return AFQ_EINVAL;
    h->step.handover.drop();            // (walkers change slots: the images do not travel with the clones)
    const bool thermal = th_thermal(h) && h->nw;              // thermal walkers: no trial determinant, G and the bins travel
    int rc = AFQ_OK;
    if (thermal) {
        h->gf.drop();
        hipSetDevice(h->device);
        if (k_comm_size(h) > 1) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: one rank only");
    } else if ((rc = need_ready(h, false))) { h->gf.drop(); return rc; }
    const int nranks = k_comm_size(h);
    if (h->nw * nranks == 1) return AFQ_OK;              // handler.py:226-227
    // a kept Green's function travels with the cloned walkers (the clone / pack kernels copy Ghalf and the cached overlap)
    // (never the spin sum alone: the clones copy Ghalf)
    const bool keep = h->gf.take() == GreensCache::FULL && h->ndet == 1;
    if ((rc = k_comb(h, r, target_weight, keep))) return rc;
    if (keep) h->gf.keep(GreensCache::FULL);
    if (!parent_ix && !total_weight_out) return AFQ_OK;  // asynchronous: nothing read back, no host sync
    double sc[8];
    if ((rc = copy_out(h, sc, h->scal, sizeof(sc)))) return rc;
    if (total_weight_out) *total_weight_out = sc[0];
    if (sc[1] < 0) AFQ_FAIL(h, AFQ_EWEIGHT, "total walker weight below 1e-8");
    if (sc[3] != 0.0) AFQ_FAIL(h, AFQ_EOVERFLOW, "more walkers moved between two ranks than the exchange slots hold");
    if (sc[6] != 0.0) AFQ_FAIL(h, AFQ_ECOMM, "communicator: a peer rank never signalled (the wait budget of afq_comm_set_timeout ran out on the device)");
    if (!parent_ix) return AFQ_OK;
    if (h->comm) return afq_comm_parent_ix(h, parent_ix);   // the global comb, [nranks * nw]
    return copy_out(h, parent_ix, h->parent_ix, sizeof(int) * h->nw);
}

int afq_popcontrol_pair_branch(afq_handle *h, const double *u, int nu, double target_weight, double min_weight,
                               double max_weight, int32_t *mult, int32_t *ndraws_out, double *total_weight_out) {
    if (h) h->scal_cache_valid = false;
    AFQ_API(h, "afq_popcontrol_pair_branch");
    if (!h) return AFQ_EINVAL;
    h->step.handover.drop();
    if (th_thermal(h)) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: pair_branch population control is not supported (comb only)");
    int rc = need_ready(h, false);
    if (rc) { h->gf.drop(); return rc; }
    if (k_comm_size(h) > 1) {
        h->gf.drop();
        AFQ_FAIL(h, AFQ_EUNSUPPORTED, "pair branching over the library-owned communicator: it does the comb only");
    }
    if (h->nw == 1) return AFQ_OK;                       // handler.py:226-227
    if (!u || nu < h->nw / 2 || !(target_weight > 0.0)) {
        h->gf.drop();
        AFQ_FAIL(h, AFQ_EINVAL, "afq_popcontrol_pair_branch: nw / 2 uniforms and a positive target weight are needed");
    }
    if ((rc = dev_grow(h, LT_WALKERS, &h->pb_u, &h->pb_u_n, (size_t)(h->nw / 2), "pair-branch uniforms"))) { h->gf.drop(); return rc; }
    AFQ_HIP(h, hipMemcpyAsync(h->pb_u, u, sizeof(double) * (size_t)(h->nw / 2), hipMemcpyHostToDevice, h->stream));
    // a kept Green's function travels with the cloned walkers, as for the comb
    const bool keep = h->gf.take() == GreensCache::FULL && h->ndet == 1;
    if ((rc = k_pair_branch(h, h->pb_u, target_weight, min_weight, max_weight, keep))) return rc;
    if (keep) h->gf.keep(GreensCache::FULL);
    if (!mult && !ndraws_out && !total_weight_out) return AFQ_OK;  // asynchronous: nothing read back, no host sync
    double sc[AFQ_NSCAL];
    if ((rc = copy_out(h, sc, h->scal, sizeof(sc)))) return rc;
    if (total_weight_out) *total_weight_out = sc[0];
    if (sc[1] < 0) AFQ_FAIL(h, AFQ_EWEIGHT, "total walker weight below 1e-8");
    if (ndraws_out) *ndraws_out = (int32_t)sc[9];
    if (!mult) return AFQ_OK;
    return copy_out(h, mult, h->parent_ix, sizeof(int) * h->nw);
}

int afq_walkers_scale_weights(afq_handle *h, double scale) {
    if (!h || scale == 0.0) return AFQ_EINVAL;
    int rc = need_ready(h, false);
    if (rc) return rc;
    return k_scale_weights(h, scale);
}

int afq_walkers_reset_weights(afq_handle *h) {
    if (!h) return AFQ_EINVAL;
    int rc = need_ready(h, false);
    if (rc) return rc;
    return k_reset_weights(h);
}

// packed walker: the entries of walker_fields (the weight included) as WalkerFields::packed_bytes lays them out, which
// starts phi | ot, ehyb, phase, eloc (c128) | unscaled_weight, detR, weight, log_detR (f64)
int afq_walker_pack_bytes(afq_handle *h, int64_t *bytes) {
    if (!h || !bytes) return AFQ_EINVAL;
    *bytes = (int64_t)walker_fields(h, WF_WEIGHT).packed_bytes();
    return AFQ_OK;
}

// What copy, pack and unpack ask first: a thermal handle has no trial determinant, its configuration stands in for one
// (the walker table then holds G, the bins, right and M0, as the header says of these three calls).
static int need_walkers(afq_handle *h) {
    if (!th_thermal(h) || !h->nw) return need_ready(h, false);
    if (h->prop_pending) AFQ_FAIL(h, AFQ_ESTATE, "a step is half done: afq_propagate_finish first");
    hipSetDevice(h->device);
    return AFQ_OK;
}

static int pack_io(afq_handle *h, int iw, char *buf, bool pack) {
    const WalkerFields f = walker_fields(h, WF_WEIGHT);
    long off = 0;
    for (int k = 0; k < f.n; ++k) {
        const WalkerFields::Entry &e = f.e[k];
        off = WalkerFields::packed_at(off, e.bytes);
        if (pack) AFQ_HIP(h, hipMemcpyAsync(buf + off, e.base + iw * e.bytes, e.bytes, hipMemcpyDeviceToDevice, h->stream));
        else AFQ_HIP(h, hipMemcpyAsync(e.base + iw * e.bytes, buf + off, e.bytes, hipMemcpyDeviceToDevice, h->stream));
        off += e.bytes;
    }
    return AFQ_OK;
}

int afq_walker_pack(afq_handle *h, int iw, void *dev_buf) {
    if (!h || !dev_buf) return AFQ_EINVAL;
    int rc = need_walkers(h);
    if (rc) return rc;
    if (iw < 0 || iw >= h->nw) AFQ_FAIL(h, AFQ_EINVAL, "walker index out of range");
    return pack_io(h, iw, (char *)dev_buf, true);
}

int afq_walker_unpack(afq_handle *h, int iw, const void *dev_buf) {
    drop_walk_caches(h);
    if (!h || !dev_buf) return AFQ_EINVAL;
    int rc = need_walkers(h);
    if (rc) return rc;
    if (iw < 0 || iw >= h->nw) AFQ_FAIL(h, AFQ_EINVAL, "walker index out of range");
    return pack_io(h, iw, (char *)dev_buf, false);
}

int afq_walkers_copy(afq_handle *h, int src, int dst) {
    drop_walk_caches(h);
    if (!h) return AFQ_EINVAL;
    int rc = need_walkers(h);
    if (rc) return rc;
    if (src < 0 || dst < 0 || src >= h->nw || dst >= h->nw) AFQ_FAIL(h, AFQ_EINVAL, "walker index out of range");
    if (src == dst) return AFQ_OK;
    const WalkerFields f = walker_fields(h, WF_WEIGHT);
    for (int k = 0; k < f.n; ++k)
        AFQ_HIP(h, hipMemcpyAsync(f.e[k].base + dst * f.e[k].bytes, f.e[k].base + src * f.e[k].bytes, f.e[k].bytes, hipMemcpyDeviceToDevice, h->stream));
    return AFQ_OK;
}

static int est_publish_args(afq_handle *h, int zero, EstPublish *pub);

// (publish_zero < 0: plain update; 0 / 1: the block's sums are handed to the host by the same summation launch, see
//  afq_estimates_update_publish)
static int estimates_update_impl(afq_handle *h, int eval_energy, int publish_zero) {
    int rc = need_ready(h, false);
    if (rc) return rc;
    if (publish_zero >= 0 && h->est_pending) AFQ_FAIL(h, AFQ_ESTATE, "afq_estimates_update_publish: a fetch is already in flight");
    if (eval_energy) {
        {
            PhaseTimer t(h, T_GREENS);
            if (h->gf.kept != GreensCache::FULL) {
                // (e.g. behind a comb that did not carry the Green's functions along: multi-determinant trials.)  It is
                // the Green's function of the CURRENT walkers, so it also is what the next step starts from: the overlaps go
                // where the end-of-step evaluation leaves them and the evaluation is kept -- with it the Coulomb vectors the
                // energy contracts below, which are the next step's force bias
                if ((rc = greens_any(h, h->ovlp_new, true))) return rc;
                if (h->gf.enabled && !(h->flags & AFQ_PROP_FREE_PROJECTION) && h->psi_stride == 0) h->gf.keep(GreensCache::FULL);
            }
            if (h->kind == AFQ_SYS_UEG || h->rdm_on) {       // (one_rdm: w.greens_function(trial) refreshes walker.G, mixed.py:212)
                if ((rc = ensure_G(h))) return rc;
                if ((rc = k_full_G(h))) return rc;
            }
        }
        PhaseTimer t(h, T_ENERGY);
        if ((rc = local_energy(h))) return rc;
    }
    if (publish_zero >= 0) {
        // (the arguments are made HERE, behind the energy evaluation: the closed-shell word that rides along is the one of
        //  the newest checking launch)
        EstPublish pub;
        if ((rc = est_publish_args(h, publish_zero, &pub))) return rc;
        if ((rc = k_estimates(h, eval_energy, false, &pub))) return rc;
        h->est_pending = true;
    } else if ((rc = k_estimates(h, eval_energy))) return rc;
    if (eval_energy && h->sf_on) {
        // sf_acc += sum_w weight_w Re two_rdm[G_w]: weight_w is what multiplies the energy in enumer (estimates_kernel)
        if (h->flags & AFQ_PROP_FREE_PROJECTION) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "mixed structure factor: importance sampling only");
        cplx *two = nullptr, *E = nullptr;                             // (the walkers' own energies stay as they are)
        if ((rc = k_ueg_sf_two(h, h->nw, &two, &E))) return rc;
        if ((rc = k_ueg_pair_sums(h, h->G, h->nw, E, two))) return rc;
        if ((rc = k_ueg_sf_wsum(h, two, h->nw, nullptr, h->weight, nullptr, h->sf_acc))) return rc;
    }
    if (h->rdm_on && !(h->flags & AFQ_PROP_FREE_PROJECTION)) {   // the free-projection branch has no RDM (mixed.py:151-175)
        if (!h->G) AFQ_FAIL(h, AFQ_ESTATE, "one_rdm: no Green's function evaluated yet");
        return k_rdm_accumulate(h);
    }
    return AFQ_OK;
}

int afq_estimates_update(afq_handle *h, int eval_energy) {
    AFQ_API(h, "afq_estimates_update");
    if (!h) return AFQ_EINVAL;
    return estimates_update_impl(h, eval_energy, -1);
}

int afq_estimates_update_publish(afq_handle *h, int eval_energy, int zero) {
    AFQ_API(h, "afq_estimates_update_publish");
    if (!h) return AFQ_EINVAL;
    return estimates_update_impl(h, eval_energy, zero ? 1 : 0);
}

int afq_estimates_rdm(afq_handle *h, int on) {
    if (!h) return AFQ_EINVAL;
    if (th_thermal(h)) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "thermal walkers: no mixed one_rdm / two_rdm");
    int rc = need_ready(h, false);
    if (rc) return rc;
    if (h->ndet > 1 || h->hirsch) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "mixed one_rdm: single-determinant trial, continuous propagator");
    h->rdm_on = on != 0;
    if (h->rdm_on && !h->rdm_acc) {
        const size_t n = (size_t)2 * h->M * h->M;
        if ((rc = dev_alloc(h, LT_WALKERS, &h->rdm_acc, n))) return rc;
        AFQ_HIP(h, hipMemsetAsync(h->rdm_acc, 0, sizeof(double) * n, h->stream));
    }
    return AFQ_OK;
}

int afq_estimates_sf(afq_handle *h, int on) {
    if (!h) return AFQ_EINVAL;
    int rc = need_ready(h, false);
    if (rc) return rc;
    if (h->kind != AFQ_SYS_UEG) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "mixed structure factor: UEG systems only");
    if (h->ndet > 1) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "mixed structure factor: single-determinant trial");
    if (on && (h->flags & AFQ_PROP_FREE_PROJECTION)) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "mixed structure factor: importance sampling only");
    h->sf_on = on != 0;
    if (h->sf_on && !h->sf_acc) {
        const size_t n = (size_t)4 * h->nq;
        if ((rc = dev_alloc(h, LT_WALKERS, &h->sf_acc, n))) return rc;
        AFQ_HIP(h, hipMemsetAsync(h->sf_acc, 0, sizeof(double) * n, h->stream));
    }
    return AFQ_OK;
}

int afq_estimates_sf_get(afq_handle *h, double *sf_out, int zero) {
    if (!h || !sf_out) return AFQ_EINVAL;
    if (!h->sf_acc) AFQ_FAIL(h, AFQ_ESTATE, "mixed structure factor accumulation is not switched on");
    hipSetDevice(h->device);
    const size_t n = (size_t)4 * h->nq;
    int rc = copy_out(h, sf_out, h->sf_acc, sizeof(double) * n);
    if (rc) return rc;
    if (zero) AFQ_HIP(h, hipMemsetAsync(h->sf_acc, 0, sizeof(double) * n, h->stream));
    return AFQ_OK;
}

int afq_estimates_rdm_get(afq_handle *h, double *rdm_out, int zero) {
    if (!h || !rdm_out) return AFQ_EINVAL;
    if (!h->rdm_acc) AFQ_FAIL(h, AFQ_ESTATE, "mixed one_rdm accumulation is not switched on");
    hipSetDevice(h->device);
    const size_t n = (size_t)2 * h->M * h->M;
    int rc = copy_out(h, rdm_out, h->rdm_acc, sizeof(double) * n);
    if (rc) return rc;
    if (zero) AFQ_HIP(h, hipMemsetAsync(h->rdm_acc, 0, sizeof(double) * n, h->stream));
    return AFQ_OK;
}

int afq_estimates_get(afq_handle *h, double *est_out, int zero) {
    if (!h || !est_out) return AFQ_EINVAL;
    const int rc = afq_estimates_get_begin(h, zero);
    return rc ? rc : afq_estimates_get_end(h, est_out);
}

// The sums of a block go to the host through ONE small kernel that writes them into mapped, coherent host memory, zeroes
// them and then publishes a sequence number there; afq_estimates_get_end polls that number.  The copy / copy / event /
// memset sequence this replaces cost ~25 us of idle device per block (rocprofv3 kernel trace: 6 us ahead of the fill
// kernel, 17 us behind it) although more work was already queued.
__global__ void est_publish_kernel(cplx *est, const double *scal, double *host_out, unsigned long long *host_seq,
                                   unsigned long long seq, int nest, int zero, const unsigned long long *closed_bad) {
    const int t = threadIdx.x;
    if (t < nest) host_out[t] = ((const double *)est)[t];
    if (t < AFQ_NSCAL) host_out[nest + t] = scal[t];
    // the closed-shell word rides along (afq_internal.h: closed_bad): a HINT for the host's choice between the one-spin-first
    // and the one-launch two-spin form of the exchange energy -- never a decision about results
    if (t == 0) host_seq[1] = closed_bad ? *closed_bad : 0ull;
    __threadfence_system();
    __syncthreads();
    if (t < nest && zero) ((double *)est)[t] = 0.0;
    if (t == 0) __hip_atomic_store(host_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

int afq_estimates_get_begin(afq_handle *h, int zero) {
    AFQ_API(h, "afq_estimates_get");
    if (!h) return AFQ_EINVAL;
    hipSetDevice(h->device);
    if (h->est_pending) AFQ_FAIL(h, AFQ_ESTATE, "afq_estimates_get_begin: a fetch is already in flight");
    EstPublish pub;
    { const int rc = est_publish_args(h, zero, &pub); if (rc) return rc; }
    if (h->est_acc_pending) {
        // sums still sitting in the per-walker accumulators: the launch that folds them in hands the block over too
        const int rc = k_estimates(h, 0, true, &pub);
        if (rc) return rc;
    } else {
        AFQ_LAUNCH(h, est_publish_kernel, dim3(1), dim3(64), 0, h->stream, h->estimates, h->scal, pub.host_out,
                   pub.host_seq, pub.seq, pub.nest, pub.zero, pub.closed_bad);
        AFQ_POST(h);
    }
    h->est_pending = true;
    return AFQ_OK;
}

// the mapped staging area, the next sequence number and the closed-shell epoch of one hand-over
static int est_publish_args(afq_handle *h, int zero, EstPublish *pub) {
    const size_t nest = 2 * (size_t)AFQ_EST_COUNT_;
    if (!h->est_stage) {
        // [nest sums | scal[AFQ_NSCAL] | sequence number], written by the device, polled by the host
        AFQ_HIP(h, hipHostMalloc((void **)&h->est_stage, sizeof(double) * (nest + AFQ_NSCAL + 2),
                                 hipHostMallocMapped | hipHostMallocCoherent));
        memset(h->est_stage, 0, sizeof(double) * (nest + AFQ_NSCAL + 2));
    }
    // the one host synchronisation of a block of steps also reports a population that collapsed in an
    // asynchronous comb (scal[2], set by comb_plan_kernel; walkers/handler.py:236-241 exits there)
    double *dev_view = nullptr;
    AFQ_HIP(h, hipHostGetDevicePointer((void **)&dev_view, h->est_stage, 0));
    ++h->est_seq;
    h->closed_epoch_pub = h->closed_epoch;                   // the newest launch whose verdict the published word can hold
    pub->host_out = dev_view; pub->host_seq = (unsigned long long *)(dev_view + nest + AFQ_NSCAL); pub->seq = h->est_seq;
    pub->scal = h->scal; pub->closed_bad = h->closed_bad; pub->nest = (int)nest; pub->zero = zero;
    return AFQ_OK;
}

int afq_estimates_get_end(afq_handle *h, double *est_out) {
    AFQ_API(h, "afq_estimates_get");
    if (!h || !est_out) return AFQ_EINVAL;
    if (!h->est_pending) AFQ_FAIL(h, AFQ_ESTATE, "afq_estimates_get_end without afq_estimates_get_begin");
    hipSetDevice(h->device);
    h->est_pending = false;
    const size_t nest = 2 * (size_t)AFQ_EST_COUNT_;
    {
        // poll the sequence number; the stream query catches a failed launch or device (no endless wait)
        const unsigned long long *seq = (const unsigned long long *)(h->est_stage + nest + AFQ_NSCAL);
        unsigned spins = 0;
        while (__atomic_load_n(seq, __ATOMIC_ACQUIRE) != h->est_seq) {
            if ((++spins & 0x3ffu) == 0) {
                const hipError_t q = hipStreamQuery(h->stream);
                if (q == hipSuccess) break;                       // everything enqueued has run
                if (q != hipErrorNotReady) AFQ_HIP(h, q);
            }
        }
        if (__atomic_load_n(seq, __ATOMIC_ACQUIRE) != h->est_seq)
            AFQ_FAIL(h, AFQ_EHIP, "estimator sums were not published by the device");
    }
    memcpy(est_out, h->est_stage, sizeof(double) * nest);
    {   // at the time of the publish, had the newest checking Green's function launch found an open-shell walker?
        const unsigned long long bad = ((const unsigned long long *)(h->est_stage + nest + AFQ_NSCAL))[1];
        h->exx_open_hint = h->closed_epoch_pub != 0 && bad >= h->closed_epoch_pub;
    }
    const double *sc = h->est_stage + nest;
    // the population-control scalars of the block ride along: afq_comm_stats right behind this call needs no synchronisation
    memcpy(h->scal_cache, sc, sizeof(double) * AFQ_NSCAL);
    h->scal_cache_valid = true;
    if (sc[2] != 0.0) AFQ_FAIL(h, AFQ_EWEIGHT, "total walker weight below 1e-8 in an earlier population control");
    if (sc[3] != 0.0) AFQ_FAIL(h, AFQ_EOVERFLOW, "population control: more walkers moved between two ranks than the "
                                                 "exchange slots hold (afq_comm_init capacity)");
    if (sc[6] != 0.0) AFQ_FAIL(h, AFQ_ECOMM, "communicator: a peer rank never signalled an all-gather row / walker slots "
                                             "(the wait budget of afq_comm_set_timeout ran out on the device)");
    return AFQ_OK;
}

// ---------------------------------------------------------------------- misc
int afq_rng_seed(afq_handle *h, uint64_t seed, uint64_t stream) {
    if (!h) return AFQ_EINVAL;
    h->rng_seed = seed; h->rng_stream = stream; h->rng_counter = 0;
    return AFQ_OK;
}

int afq_rng_normal(afq_handle *h, double *out, int64_t n) {
    if (!h || !out || n < 1) return AFQ_EINVAL;
    hipSetDevice(h->device);
    DevTemp<double> tmp;
    int rc = dev_temp(h, tmp, (size_t)n);
    if (!rc) rc = k_rng_normal_into(h, tmp, (long)n);
    if (!rc) rc = copy_out(h, out, tmp, sizeof(double) * (size_t)n);
    return rc;
}

int afq_rng_philox4x32(afq_handle *h, const uint32_t *ctr_key, uint32_t *out, int n) {
    if (!h || !ctr_key || !out || n < 1) return AFQ_EINVAL;
    hipSetDevice(h->device);
    DevTemp<uint32_t> in_d, out_d;
    int rc = dev_temp(h, in_d, (size_t)6 * n, ctr_key);
    if (!rc) rc = dev_temp(h, out_d, (size_t)4 * n);
    if (!rc) rc = k_philox_raw(h, in_d, out_d, n);
    if (!rc) rc = copy_out(h, out, out_d, sizeof(uint32_t) * 4 * (size_t)n);
    return rc;
}

int afq_debug(afq_handle *h, int sync_every_launch, int markers) {
    if (!h) return AFQ_EINVAL;
    h->debug_sync = sync_every_launch != 0;
    h->debug_markers = markers != 0;
    return AFQ_OK;
}

// Readable from a watchdog thread while the owning thread is blocked inside a synchronising call: touches
// host memory only (no HIP call, no lock).
int afq_last_launch(afq_handle *h, char *buf, int len, uint64_t *queued, uint64_t *retired) {
    if (!h || !buf || len < 1) return AFQ_EINVAL;
    const unsigned long long n = h->n_launch, r = h->retired ? *h->retired : 0ull;
    if (queued) *queued = n;
    if (retired) *retired = h->debug_markers ? r : 0ull;
    std::string txt = std::string("api=") + (h->crumb_api ? h->crumb_api : "") + " queued=" + std::to_string(n);
    if (h->debug_markers) {
        txt += " retired=" + std::to_string(r);
        if (r < n && h->crumb_name[r & 63] && n - r <= 64) txt += std::string(" first-unretired=") + h->crumb_name[r & 63];
    }
    txt += " last:";
    for (unsigned long long i = n > 8 ? n - 8 : 0; i < n; ++i)
        txt += std::string(" ") + (h->crumb_name[i & 63] ? h->crumb_name[i & 63] : "?");
    snprintf(buf, (size_t)len, "%s", txt.c_str());
    return AFQ_OK;
}

int afq_counters_ext(afq_handle *h, int64_t *out, int n, int reset) {
    if (!h || !out || n < 0) return AFQ_EINVAL;
    hipSetDevice(h->device);
    unsigned long long c[AFQ_NCOUNTERS];
    int rc = copy_out(h, c, h->counters, sizeof(c));
    if (rc) return rc;
    for (int i = 0; i < n; ++i) out[i] = i < AFQ_NCOUNTERS ? (int64_t)c[i] : 0;
    if (reset) AFQ_HIP(h, hipMemsetAsync(h->counters, 0, sizeof(c), h->stream));
    return AFQ_OK;
}

int afq_counters(afq_handle *h, int64_t *out, int reset) { return afq_counters_ext(h, out, 4, reset); }

int afq_enable_timers(afq_handle *h, int on) {
    if (!h) return AFQ_EINVAL;
    h->timers_on = on != 0;
    return AFQ_OK;
}

int afq_timers(afq_handle *h, double *out_ms, int reset) {
    if (!h || !out_ms) return AFQ_EINVAL;
    for (int i = 0; i < T_COUNT; ++i) { out_ms[i] = h->t_ms[i]; if (reset) h->t_ms[i] = 0.0; }
    return AFQ_OK;
}

// ---------------------------------------------------------------- discrete Hirsch propagator
static int hirsch_buffers(afq_handle *h) {
    if (h->hs_oinv) return AFQ_OK;
    const size_t n = h->nw, nmax = h->na > h->nb ? h->na : h->nb;
    int rc;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->hs_oinv, n * 2 * nmax * nmax))) return rc;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->hs_u, n * h->M))) return rc;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->hs_fields, n * h->M))) return rc;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->hs_used, n))) return rc;
    if ((rc = dev_alloc(h, LT_WALKERS, &h->hs_alive0, n))) return rc;
    AFQ_HIP(h, hipMemsetAsync(h->hs_alive0, 0, sizeof(int) * n, h->stream));
    return AFQ_OK;
}

static int hirsch_ready(afq_handle *h) {
    int rc = need_ready(h, true);
    if (rc) return rc;
    if (!h->hirsch) AFQ_FAIL(h, AFQ_ESTATE, "the discrete Hirsch propagator is not set");
    return hirsch_buffers(h);
}

int afq_set_propagator_hirsch(afq_handle *h, const double *bt2, double dt, int charge_decomposition) {
    drop_walk_caches(h);
    if (!h || !bt2 || dt <= 0) return AFQ_EINVAL;
    if (h->kind != AFQ_SYS_HUBBARD) AFQ_FAIL(h, AFQ_ESTATE, "the Hirsch transformation needs a Hubbard system");
    if (h->ndet > 1) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "Hirsch propagator: single-determinant trials");
    hipSetDevice(h->device);
    int rc;
    if ((rc = dev_upload(h, LT_HANDLE, &h->BH1, bt2, (size_t)2 * h->M * h->M))) return rc;
    h->bh1_real = true;         // (expm of a real hopping matrix: the one-body GEMM then needs two real products per pair)
    for (size_t i = 0, n = (size_t)2 * h->M * h->M; i < n && h->bh1_real; ++i) h->bh1_real = bt2[2 * i + 1] == 0.0;
    h->bh1_same = false;
    cache_of(h)->BH1.clear();
    if ((rc = step_operands(h))) return rc;
    // propagation/hubbard.py:66-82
    typedef std::complex<double> C;
    C gamma, auxf[2][2], wfac[2];
    const double e = std::exp(-0.5 * dt * h->U);
    if (charge_decomposition) {
        gamma = std::acosh(C(e, 0.0));
        auxf[0][0] = auxf[0][1] = std::exp(gamma);
        auxf[1][0] = auxf[1][1] = std::exp(-gamma);
        wfac[0] = std::exp(0.5 * dt * h->U) * std::exp(-gamma);
        wfac[1] = std::exp(0.5 * dt * h->U) * std::exp(gamma);
    } else {
        gamma = C(std::acosh(std::exp(0.5 * dt * h->U)), 0.0);
        auxf[0][0] = std::exp(gamma); auxf[0][1] = std::exp(-gamma);
        auxf[1][0] = std::exp(-gamma); auxf[1][1] = std::exp(gamma);
        wfac[0] = wfac[1] = C(1.0, 0.0);
    }
    for (int x = 0; x < 2; ++x) {
        h->hs_wfac[x] = cmake(wfac[x].real(), wfac[x].imag());
        for (int sp = 0; sp < 2; ++sp) {
            const C f = auxf[x][sp] * e, d = f - 1.0;
            h->hs_auxf[x][sp] = cmake(f.real(), f.imag());
            h->hs_delta[x][sp] = cmake(d.real(), d.imag());
        }
    }
    h->hs_gamma = cmake(gamma.real(), gamma.imag());
    h->hs_charge = charge_decomposition != 0;
    h->hs_direct = false;
    if (!h->mf_shift) {
        std::vector<double> z(2 * (size_t)h->K, 0.0);
        if ((rc = dev_upload(h, LT_HANDLE, &h->mf_shift, z.data(), (size_t)h->K))) return rc;
    }
    h->dt = dt; h->sqrt_dt = std::sqrt(dt);
    h->flags = 0; h->nv = 1; h->vhs_diag = true;
    h->hirsch = true; h->have_prop = true;
    return AFQ_OK;
}

int afq_hirsch_kinetic(afq_handle *h) {
    drop_walk_caches(h);
    if (!h) return AFQ_EINVAL;
    int rc = hirsch_ready(h);
    if (rc) return rc;
    if ((rc = k_hirsch_alive(h, 0))) return rc;                 // walkers the driver propagates (|w| > 1e-8)
    return k_hirsch_kinetic(h);
}

int afq_hirsch_two_body(afq_handle *h, const double *u, int32_t *fields_out, int32_t *used_out) {
    drop_walk_caches(h);
    if (!h || !u) return AFQ_EINVAL;
    int rc = hirsch_ready(h);
    if (rc) return rc;
    AFQ_HIP(h, hipMemcpyAsync(h->hs_u, u, sizeof(double) * (size_t)h->nw * h->M, hipMemcpyHostToDevice, h->stream));
    if ((rc = k_hirsch_alive(h, 1))) return rc;                 // if abs(walker.weight) > 0 (hubbard.py:308)
    if ((rc = k_hirsch_two_body(h))) return rc;
    if (fields_out && (rc = copy_out(h, fields_out, h->hs_fields, sizeof(int) * (size_t)h->nw * h->M))) return rc;
    if (used_out && (rc = copy_out(h, used_out, h->hs_used, sizeof(int) * (size_t)h->nw))) return rc;
    return AFQ_OK;
}

int afq_hirsch_finish(afq_handle *h, double eshift) {
    drop_walk_caches(h);
    if (!h) return AFQ_EINVAL;
    int rc = hirsch_ready(h);
    if (rc) return rc;
    if ((rc = k_hirsch_alive(h, 1))) return rc;                 // if abs(walker.weight.real) > 0 (:310)
    if ((rc = k_hirsch_kinetic(h))) return rc;
    if ((rc = k_hirsch_eshift(h, std::exp(h->dt * eshift)))) return rc;
    return k_alive(h);
}

int afq_propagate_hirsch(afq_handle *h, double eshift) {
    AFQ_API(h, "afq_propagate_hirsch");
    drop_walk_caches(h);
    if (!h) return AFQ_EINVAL;
    int rc = hirsch_ready(h);
    if (rc) return rc;
    if ((rc = k_hirsch_alive(h, 0))) return rc;
    if ((rc = k_hirsch_kinetic(h))) return rc;
    if ((rc = k_rng_uniform(h, h->hs_u, (long)h->nw * h->M))) return rc;
    if ((rc = k_hirsch_alive(h, 1))) return rc;
    if ((rc = k_hirsch_two_body(h))) return rc;
    if ((rc = k_hirsch_alive(h, 1))) return rc;
    if ((rc = k_hirsch_kinetic(h))) return rc;
    if ((rc = k_hirsch_eshift(h, std::exp(h->dt * eshift)))) return rc;
    return k_alive(h);
}

int afq_hirsch_single_site(afq_handle *h, int on) {
    if (!h) return AFQ_EINVAL;
    if (!h->hirsch) AFQ_FAIL(h, AFQ_ESTATE, "afq_set_propagator_hirsch first");
    if (!on && h->nbp > 0) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "the direct Hirsch update records no field history (hubbard.py:222-275)");
    h->hs_direct = !on;
    return AFQ_OK;
}

int afq_hirsch_free_projection(afq_handle *h, int on) {
    if (!h) return AFQ_EINVAL;
    if (!h->hirsch) AFQ_FAIL(h, AFQ_ESTATE, "afq_set_propagator_hirsch first");
    if (on && h->nbp > 0) AFQ_FAIL(h, AFQ_EUNSUPPORTED, "no field history in free projection");
    // the estimators (mixed.py:151-175) and the re-orthogonalisation (walkers/handler.py:176-180) read the flag
    if (on) h->flags |= AFQ_PROP_FREE_PROJECTION; else h->flags &= ~AFQ_PROP_FREE_PROJECTION;
    return AFQ_OK;
}

int afq_propagate_hirsch_free(afq_handle *h, const double *u, int32_t *fields_out, double eshift) {
    AFQ_API(h, "afq_propagate_hirsch_free");
    drop_walk_caches(h);
    if (!h) return AFQ_EINVAL;
    int rc = hirsch_ready(h);
    if (rc) return rc;
    if (!(h->flags & AFQ_PROP_FREE_PROJECTION)) AFQ_FAIL(h, AFQ_ESTATE, "afq_hirsch_free_projection(h, 1) first");
    if ((rc = k_hirsch_alive(h, 0))) return rc;                   // the driver's test |weight| > 1e-8 (qmc/afqmc.py:232)
    if (u) AFQ_HIP(h, hipMemcpyAsync(h->hs_u, u, sizeof(double) * (size_t)h->nw * h->M, hipMemcpyHostToDevice, h->stream));
    else if ((rc = k_rng_uniform(h, h->hs_u, (long)h->nw * h->M))) return rc;
    if ((rc = k_hirsch_free(h, eshift))) return rc;
    if (fields_out && (rc = copy_out(h, fields_out, h->hs_fields, sizeof(int) * (size_t)h->nw * h->M))) return rc;
    return k_alive(h);
}

int afq_walkers_det_weights(afq_handle *h, double *weights_out) {
    if (!h || !weights_out) return AFQ_EINVAL;
    if (!h->nw) AFQ_FAIL(h, AFQ_ESTATE, "no walkers allocated");
    hipSetDevice(h->device);
    if (h->ndet <= 1) AFQ_FAIL(h, AFQ_ESTATE, "single-determinant trial: the overlap is the only weight");
    return copy_out(h, weights_out, h->detw, sizeof(cplx) * (size_t)h->nw * h->ndet);
}

int afq_kernel_trace(afq_handle *h, int on) {
    if (!h) return AFQ_EINVAL;
    // on == 1: every kind; on > 1: bit (k + 1) selects kind k, e.g. 2 = AFQ_K_PROPAGATOR only; 0: off
    h->ktrace_mask = on == 1 ? ~0u : on > 1 ? (unsigned)on >> 1 : 0u;
    if (on) for (int k = 0; k < AFQ_K_COUNT; ++k) { h->ktrace_used[k] = 0; h->ktrace_seen[k] = 0; }
    return AFQ_OK;
}

int afq_kernel_trace_stride(afq_handle *h, int kind, int stride) {
    if (!h || stride < 1 || kind < 0 || kind >= AFQ_K_COUNT) return AFQ_EINVAL;
    h->ktrace_stride[kind] = stride;
    return AFQ_OK;
}

int afq_kernel_trace_get(afq_handle *h, int kind, double *ms_out, int max_n, int *n_out) {
    if (!h || !n_out || kind < 0 || kind >= AFQ_K_COUNT || (max_n > 0 && !ms_out)) return AFQ_EINVAL;
    hipSetDevice(h->device);
    AFQ_HIP(h, hipStreamSynchronize(h->stream));
    const int n = h->ktrace_used[kind] < max_n ? h->ktrace_used[kind] : max_n;
    for (int i = 0; i < n; ++i) {
        float f = 0;
        AFQ_HIP(h, hipEventElapsedTime(&f, h->ktrace_ev[kind][2 * i], h->ktrace_ev[kind][2 * i + 1]));
        ms_out[i] = f;
    }
    *n_out = h->ktrace_used[kind];
    return AFQ_OK;
}

int afq_launch_trace(afq_handle *h, int on) {
    if (!h) return AFQ_EINVAL;
    hipSetDevice(h->device);
    if (h->ltrace_open) afq_launch_trace_mark(h, nullptr);
    if (on) h->ltrace_name.clear();
    h->ltrace_on = on != 0;
    return AFQ_OK;
}

int afq_launch_trace_get(afq_handle *h, char *names_out, int names_len, double *total_ms, int64_t *launches,
                         int max_names, int *n_out) {
    if (!h || !n_out || (max_names > 0 && (!names_out || !total_ms || !launches))) return AFQ_EINVAL;
    hipSetDevice(h->device);
    if (h->ltrace_open) afq_launch_trace_mark(h, nullptr);
    AFQ_HIP(h, hipStreamSynchronize(h->stream));
    std::vector<std::string> names;
    std::vector<double> ms;
    std::vector<int64_t> cnt;
    for (size_t i = 0; i < h->ltrace_name.size(); ++i) {
        float f = 0;
        AFQ_HIP(h, hipEventElapsedTime(&f, h->ltrace_ev[2 * i], h->ltrace_ev[2 * i + 1]));
        size_t k = 0;
        while (k < names.size() && names[k] != h->ltrace_name[i]) ++k;
        if (k == names.size()) { names.push_back(h->ltrace_name[i]); ms.push_back(0.0); cnt.push_back(0); }
        ms[k] += f; cnt[k] += 1;
    }
    *n_out = (int)names.size();
    size_t at = 0;
    for (int k = 0; k < (int)names.size() && k < max_names; ++k) {
        if (at + names[k].size() + 1 > (size_t)names_len) AFQ_FAIL(h, AFQ_EINVAL, "afq_launch_trace_get: names buffer too small");
        memcpy(names_out + at, names[k].c_str(), names[k].size() + 1);
        at += names[k].size() + 1;
        total_ms[k] = ms[k]; launches[k] = cnt[k];
    }
    return AFQ_OK;
}

int afq_propagator_issued_flops(afq_handle *h, double *open_per_walker, double *closed_per_walker) {
    if (!h || !open_per_walker || !closed_per_walker) return AFQ_EINVAL;
    *open_per_walker = h->step.issued.open;
    *closed_per_walker = h->step.issued.closed;
    return AFQ_OK;
}

int afq_kernel_issued_flops(afq_handle *h, int kind, double *flops_out) {
    if (!h || !flops_out || kind < 0 || kind >= AFQ_K_COUNT) return AFQ_EINVAL;
    *flops_out = h->issued_flops[kind];
    return AFQ_OK;
}

}  // extern "C"
