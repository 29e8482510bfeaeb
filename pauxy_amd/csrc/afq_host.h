// Host-side helpers shared by the translation units that sequence the kernels (afq_api.hip, afq_windows.hip).
#pragma once
#include "afq_internal.h"

template <class T> static int dev_alloc(afq_handle *h, T **p, size_t n) {
    if (*p) { hipFree(*p); *p = nullptr; }
    if (n == 0) return AFQ_OK;
    hipError_t e = hipMalloc((void **)p, n * sizeof(T));
    if (e != hipSuccess) { h->err = std::string("hipMalloc: ") + hipGetErrorString(e); return AFQ_ENOMEM; }
    return AFQ_OK;
}

template <class T> static int dev_upload(afq_handle *h, T **p, const void *src, size_t n) {
    int rc = dev_alloc(h, p, n);
    if (rc) return rc;
    if (n) AFQ_HIP(h, hipMemcpy(*p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return AFQ_OK;
}

template <class T> static void dev_free(T *&p) { if (p) { hipFree(p); p = nullptr; } }

#define AFQ_API(h, name) do { if (h) (h)->crumb_api = name; } while (0)

static inline int need_ready(afq_handle *h, bool prop) {
    if (!h->kind || !h->have_trial || !h->nw) AFQ_FAIL(h, AFQ_ESTATE, "system, trial and walkers must be set");
    if (prop && !h->have_prop) AFQ_FAIL(h, AFQ_ESTATE, "propagator not set");
    if (h->prop_pending) AFQ_FAIL(h, AFQ_ESTATE, "a step is half done: afq_propagate_finish first");
    hipSetDevice(h->device);
    return AFQ_OK;
}

static inline int ensure_G(afq_handle *h) {
    if (!h->G) {
        int rc = dev_alloc(h, &h->G, (size_t)2 * h->M * h->M * h->nw);
        if (rc) return rc;
    }
    return AFQ_OK;
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
