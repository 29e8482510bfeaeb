// Device memory of the handle, owned by lifetime.
//
// Every device block has exactly ONE owning slot: a pointer field of the handle (or of an afq_handle::DetOps), entered in
// the registry under the lifetime that ends it when it is allocated -- by dev_alloc / dev_upload (allocate or replace),
// dev_ensure (allocate if null) or dev_grow (at least n elements, with a length field).  Nothing else allocates into a
// handle field, and nothing frees one but these three and DevMem::release:
//   LT_HANDLE   afq_destroy              estimates, counters, closed_bad, scal, zero_page, BH1, mf_shift
//   LT_SYSTEM   a new afq_set_system_*   the Hamiltonian's operands and what is derived from them alone
//   LT_TRIAL    a new system or trial    dets[d].* (below), psicT, coeffs, msd_psicT*, psiB_cT
//   LT_WALKERS  afq_walkers_alloc        everything sized by nw, the windows configured after the walkers included
// release(lifetime) frees every block of that lifetime, nulls its slot and zeroes the length that goes with it, so an
// "ensure" or "grow" of a later configuration never meets a block sized for an earlier one.
//
// Views are never registered and never allocated through:
//   ghalf, vbias                 offsets into ghalf_all / vbias_all (the selected determinant's slice)
//   psi, psic, rH1, rchol_re/im, rchol_frag*, atil, rchol_same
//                                copies of dets[cur_det], refreshed by select_det and by nothing else; dets[] is the
//                                only owner of the trial's operands (one element for a single determinant).  An upload
//                                writes to dets[cur_det] and then refreshes the view.
//   dets[d].atil[1]              equals atil[0] when both spins share the half-rotated vectors: owned by atil[0] alone
//   Lent<>                       points a VIEW field (or phi / G / BH1 / xs / ot / detR, which no release runs under)
//                                at foreign memory for a scope; it is never handed a slot that release would free
// The communicator (afq_comm_state) and the plane-wave tables (ueg_fast) own their memory in their own structs.
//
// Every block here is allocated by guard_alloc and freed by guard_free (dev_guard.h): with AFQ_DEBUG_GUARD unset these are
// hipMalloc and hipFree; set, the block sits between two bands that are checked when it is freed.  The plane-wave tables
// allocate the same way.  The communicator's windows and exchange buffers (k_comm.hip) stay out of the guard mode: they are
// exported to peers, which address them by their base.
#pragma once
#include "dev_guard.h"
#include <vector>

enum Lifetime { LT_HANDLE = 0, LT_SYSTEM, LT_TRIAL, LT_WALKERS, LT_COUNT };

struct DevMem {
    struct Slot { void **p; size_t *len; };
    std::vector<Slot> owned[LT_COUNT];
    long allocations = 0;       // blocks allocated so far (afq_thermal_device_allocations: a test that nothing allocates per call)
    GuardCfg guard;             // AFQ_DEBUG_GUARD / AFQ_DEBUG_GUARD_BYTES as afq_create found them

    // frees what the slot holds, allocates bytes (0: leaves it null) and enters the slot under lt; *len is zeroed.  floating:
    // the element type is double, cplx or float (what the guard mode's poison goes by); what: the block's name in its log
    hipError_t replace(Lifetime lt, void **p, size_t bytes, size_t *len, bool floating = false, const char *what = "device buffer") {
        std::vector<Slot> &v = owned[lt];
        size_t i = 0;
        while (i < v.size() && v[i].p != p) ++i;
        if (i == v.size()) v.push_back({p, len});
        if (*p) { guard_free(*p); *p = nullptr; }
        if (len) *len = 0;
        if (!bytes) return hipSuccess;
        const hipError_t e = guard_alloc(guard, p, bytes, floating, what, this);
        if (e != hipSuccess) *p = nullptr;
        else ++allocations;
        return e;
    }
    void release(Lifetime lt) {
        for (const Slot &s : owned[lt]) {
            if (*s.p) { guard_free(*s.p); *s.p = nullptr; }
            if (s.len) *s.len = 0;
        }
        owned[lt].clear();
    }
};

// A per-call device buffer: every way out of the scope frees it.
template <class T> struct DevTemp {
    T *p = nullptr;
    DevTemp() = default;
    DevTemp(const DevTemp &) = delete;
    DevTemp &operator=(const DevTemp &) = delete;
    ~DevTemp() { if (p) guard_free(p); }
    // mem: the handle's memory, whose guard mode the buffer takes (none: a plain allocation)
    hipError_t alloc(size_t n, const DevMem *mem = nullptr, const char *what = "per-call buffer") {
        return guard_alloc(mem ? mem->guard : GuardCfg(), (void **)&p, n * sizeof(T), DevFloating<T>::value, what, mem);
    }
    operator T *() const { return p; }
};
