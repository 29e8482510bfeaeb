// What one walker carries: THE list of the device arrays that make up a walker.  Everything that moves a walker loops
// over it -- afq_walkers_copy, afq_walker_pack / unpack and afq_walker_pack_bytes (afq_api.hip), clone_kernel
// (k_small.hip), the exchange slots of the communicator (k_comm.hip).  State a walker gains is one line in walker_fields.
#pragma once
#include "afq_internal.h"

struct WalkerFields {
    static constexpr int MAX = 24;
    struct Entry { char *base; long bytes; };       // walker w's part of the array: `bytes` bytes at base + w * bytes
    int n = 0;
    int ghalf = -1;                                 // the entry that is the cached Ghalf (the unpack's closed-shell check); -1: not carried
    Entry e[MAX];

    // Packed form of one walker (a host pack buffer, an exchange slot): the entries in order, each at the next multiple of
    // the unit it is copied in, the whole rounded up to 16 bytes.
    static __host__ __device__ long unit(long bytes) { return bytes % 16 == 0 ? 16 : bytes % 8 == 0 ? 8 : 4; }
    static __host__ __device__ long packed_at(long off, long bytes) { return (off + unit(bytes) - 1) & ~(unit(bytes) - 1); }
    __host__ __device__ long packed_bytes() const {
        long off = 0;
        for (int k = 0; k < n; ++k) off = packed_at(off, e[k].bytes) + e[k].bytes;
        return (off + 15) & ~15L;
    }
};

// The groups a caller can ask for on top of what the handle's state switches on (back-propagation, walker.G, thermal):
enum {
    WF_WEIGHT = 1,      // the weight: the host copy and the host pack only (the comb resets it, the pair-branch plan writes it)
    WF_GREENS = 2,      // the cached Green's function, when the caller kept one
    WF_GSUM = 4,        // its spin sum and ...
    WF_GDIAG = 8,       // ... its diagonal sums: a clone inside the rank only, each when current
};

// Order: the packed prefix (phi, ot, ehyb, phase, eloc, unscaled, detR, weight, log_detR) is what callers of
// afq_walker_pack index into; behind it the order is free.  Nothing is carried for the extra determinants of a
// multi-determinant trial.
inline WalkerFields walker_fields(const afq_handle *h, int want) {
    WalkerFields f;
    auto add = [&f](auto *p, size_t n) { f.e[f.n++] = {(char *)p, (long)(sizeof(*p) * n)}; };
    const size_t per = (size_t)h->M * h->nt, mm2 = (size_t)2 * h->M * h->M;
    add(h->phi, per); add(h->ot, 1); add(h->ehyb, 1); add(h->phase, 1); add(h->eloc, 1);
    add(h->unscaled, 1); add(h->detR, 1);
    if (want & WF_WEIGHT) add(h->weight, 1);
    add(h->log_detR, 1);
    if (h->nbp > 0) {       // phi_old, the field history, the two running weight factors, FieldConfig.step (walkers/walker.py:89-90)
        add(h->phi_old, per); add(h->bp_hist, (size_t)h->nbp * h->K); add(h->bp_ph, 1); add(h->bp_cos, 1); add(h->bp_n, 1);
    }
    if (h->rdm_on && h->G) add(h->G, mm2);          // walker.G is walker state for the mixed one_rdm (estimators/mixed.py:226-229)
    if (want & WF_GREENS) { f.ghalf = f.n; add(h->ghalf, per); add(h->ovlp_new, 1); }
    if (want & WF_GSUM) add(h->ghalf_sum, (size_t)h->na * h->M);
    if (want & WF_GDIAG) add(h->gdiag, (size_t)2 * h->gdiag_parts * h->M);
    if (h->th_kind == TH_REAL) { add(h->th_G, mm2); add(h->th_stack, mm2 * h->th_nbins); }   // thermal walkers: G and the bins
    if (th_complex(h)) {                  // continuous fields: complex G and bins, the current bin's product, M0
        add(h->thc_G, mm2); add(h->thc_stack, mm2 * h->th_nbins); add(h->thc_right, mm2); add(h->thc_M0, 2);
    }
    return f;
}

// `bytes` bytes from src to dst in units of 16, 8 or 4 bytes, by the threads t0, t0 + stride, ...
__device__ __forceinline__ void walker_field_copy(char *dst, const char *src, long bytes, long t0, long stride) {
    if (bytes % 16 == 0)
        for (long i = t0; i < bytes / 16; i += stride) ((double2 *)dst)[i] = ((const double2 *)src)[i];
    else if (bytes % 8 == 0)
        for (long i = t0; i < bytes / 8; i += stride) ((double *)dst)[i] = ((const double *)src)[i];
    else
        for (long i = t0; i < bytes / 4; i += stride) ((int *)dst)[i] = ((const int *)src)[i];
}
