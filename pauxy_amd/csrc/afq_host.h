// Host-side helpers shared by the translation units that sequence the kernels (afq_api.hip, afq_windows.hip).
#pragma once
#include "afq_internal.h"

#define AFQ_API(h, name) do { if (h) (h)->crumb_api = name; } while (0)

static inline int need_ready(afq_handle *h, bool prop) {
    if (!h->kind || !h->have_trial || !h->nw) AFQ_FAIL(h, AFQ_ESTATE, "system, trial and walkers must be set");
    if (prop && !h->have_prop) AFQ_FAIL(h, AFQ_ESTATE, "propagator not set");
    if (h->prop_pending) AFQ_FAIL(h, AFQ_ESTATE, "a step is half done: afq_propagate_finish first");
    hipSetDevice(h->device);
    return AFQ_OK;
}

static inline int ensure_G(afq_handle *h) {
    return dev_ensure(h, LT_WALKERS, &h->G, (size_t)2 * h->M * h->M * h->nw);
}

static inline int copy_out(afq_handle *h, void *host, const void *dev, size_t bytes) {
    if (!host) return AFQ_OK;
    AFQ_HIP(h, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, h->stream));
    AFQ_HIP(h, hipStreamSynchronize(h->stream));
    return AFQ_OK;
}

static inline int build_vhs(afq_handle *h) {
    if (h->kind == AFQ_SYS_GENERIC) return k_vhs_generic(h);
    if (h->kind == AFQ_SYS_HUBBARD) return k_vhs_hubbard(h);
    return k_vhs_ueg(h);
}

static inline int apply_exp(afq_handle *h, const cplx *vhs) {
    if (h->vhs_diag) return k_apply_exponential_diag(h, vhs);
    return k_apply_exponential(h, vhs);
}
