"""Launch behaviour of the cached Green's function: which Green's function kernels, spin sums, closed-shell checks and
force-bias contractions a step launches after each thing a driver can do between two steps.  Every case sets the walkers,
takes one step, then traces ONE segment -- the action and one more step -- under afq_launch_trace and compares the
launches that belong to the Green's function and its by-products, name -> count, with the table below.  The tables are
what the library launched before the cache's bookkeeping got one owner (recorded with this file, unchanged, on that
commit): a missed invalidation shows as a missing launch, a lost reuse as an extra one.  What these paths compute is held
by test_gpu_overlap.py, test_gpu_c3_traj.py and the trajectory suites; no tolerance here.

Shapes, the smallest that reach each path: generic closed-shell trial M = 24, K = 30, 5 + 5 electrons with 64 walkers
(spin sum and closed-shell verdict need more than 32) and with 24 (no spin sum); a 2-determinant trial M = 12, K = 10,
3 + 3, 8 walkers (per-determinant partials, nothing kept across a comb); Hubbard with continuous fields, 8 x 8 sites,
46 + 46 electrons, 8 walkers (the large path with the diagonal sums; 46 is the first count past the small kernel)."""
import ctypes
import functools
import re

import numpy
import pytest

from pauxy_amd import _lib as L

pytestmark = pytest.mark.gpu

# the Green's function kernels of both paths, the spin sum, the closed-shell check, the force-bias contractions
OURS = re.compile(r"greens_|gj_|det_combine_kernel|k_greens_big:|ghalf_sum_kernel|ghalf_closed_check_kernel|"
                  r"force_bias_generic_impl|msd_gbar")


@functools.lru_cache(maxsize=None)
def model_of(config):
    """-> (RefModel, nw, walkers [nw, M, nt])"""
    from oracle import afqmc_ref as ref
    from pauxy_amd import systems, trial as trial_mod
    from pauxy_amd.propagation import setup
    rng = numpy.random.RandomState(17)
    if config in ('rhf64', 'rhf24'):
        from tests.test_gpu_sizes import build
        M, K, n = 24, 30, 5
        model, _ = build(M, K, n, n, False)
        nw = 64 if config == 'rhf64' else 24
        # closed-shell walkers: the beta block is the alpha block, bit for bit
        a = model.psi[None, :, :n] + 0.05 * (rng.rand(nw, M, n) + 1j * rng.rand(nw, M, n))
        return model, nw, numpy.concatenate([a, a], axis=2)
    if config == 'msd2':
        M, K, n, ndet, nw, dt = 12, 10, 3, 2, 8, 0.005
        s = systems.synthetic_generic(M, K, (n, n), seed=7)
        t0 = trial_mod.rhf_trial_generic(s)
        dets = numpy.array([t0.psi + (0.0 if d == 0 else 0.05) * (rng.rand(M, 2 * n) + 1j * rng.rand(M, 2 * n))
                            for d in range(ndet)])
        coeffs = (rng.rand(ndet) + 0.2) * numpy.exp(1j * rng.rand(ndet))
        t = trial_mod.MultiDetTrial(s, (coeffs, dets), init=t0.psi)
        BH1, mf = setup.generic_propagator_arrays(s, t, dt)
        model = ref.RefModel('generic_msd', M, n, n, dets, BH1, mf, dt, coeffs=coeffs, hs_pot=s.hs_pot,
                             H1=numpy.array([s.H1[0], s.H1[1]]).astype(complex), ecore=s.ecore)
        return model, nw, t0.psi[None] + 0.05 * (rng.rand(nw, M, 2 * n) + 1j * rng.rand(nw, M, 2 * n))
    assert config == 'hub8x8', config
    nx, n, nw, dt = 8, 46, 8, 0.01
    s = systems.Hubbard(nx, nx, n, n, 4.0)
    t = trial_mod.uhf_trial_hubbard(s, ueff=0.4)
    BH1, mf = setup.hubbard_propagator_arrays(s, t, dt, True)
    model = ref.RefModel('hubbard', nx * nx, n, n, t.psi, BH1, mf, dt, U=4.0, H1=s.T.astype(complex))
    return model, nw, t.psi[None] + 0.05 * (rng.rand(nw, nx * nx, 2 * n) + 1j * rng.rand(nw, nx * nx, 2 * n))


def comb(dev, model=None):
    """a population that forces clones: a quarter of the walkers dead, a quarter of triple weight"""
    w = numpy.ones(dev.nw)
    w[0::4] = 3.0
    w[1::4] = 0.0
    dev.set(L.F_WEIGHT, w)
    pix, _ = dev.popcontrol_comb(0.3, dev.nw)
    assert len(set(pix)) < dev.nw           # some walker was cloned over another


def device_ptr(dev, model=None):
    ptr, per = ctypes.c_void_p(), ctypes.c_int64()
    assert dev.lib.afq_walkers_device_ptr(dev.h, L.F_GHALF, ctypes.byref(ptr), ctypes.byref(per)) == 0


def bp_window(dev, model):
    dev.bp_update(model.psi, 5, None)


# scenario -> (announce the first step with estimates_fuse_next, back-propagation steps, action of the segment)
SCENARIOS = {
    'nothing': (False, 0, lambda dev, model: None),
    'reortho': (False, 0, lambda dev, model: dev.reortho()),
    'comb': (False, 0, comb),
    'set_phi': (False, 0, lambda dev, model: dev.set(L.F_PHI, dev.get(L.F_PHI))),
    'estimates_update': (False, 0, lambda dev, model: dev.estimates_update(True)),
    # the first step was announced with estimates_fuse_next: it leaves overlap + spin sum (or diagonal sums) only
    'fused_nothing': (True, 0, lambda dev, model: None),
    'fused_local_energy': (True, 0, lambda dev, model: dev.local_energy()),
    'fused_get_ghalf': (True, 0, lambda dev, model: dev.get(L.F_GHALF)),
    'fused_reortho': (True, 0, lambda dev, model: dev.reortho()),
    'fused_comb': (True, 0, comb),
    # ... and here the traced step is the announced one
    'fuse_next': (False, 0, lambda dev, model: dev.estimates_fuse_next()),
    'device_ptr': (False, 0, device_ptr),
    'bp_window': (False, 2, bp_window),
}
# (the device back-propagates Hubbard systems with discrete fields only, and a multi-determinant handle has its own window)
CASES = [(c, s) for c in ('rhf64', 'rhf24', 'msd2', 'hub8x8') for s in SCENARIOS
         if not (s == 'bp_window' and c in ('msd2', 'hub8x8'))]


def trace_segment(config, scenario):
    """set PHI, one step (as many as the window holds with back-propagation on), then the traced segment: the action and
    one more step -> {name: launches} of the Green's function's launches"""
    from tests.helpers import make_device
    fuse_first, nbp, action = SCENARIOS[scenario]
    model, nw, phis = model_of(config)
    dev = make_device(model, nw)
    try:
        dev.rng_seed(7)
        dev.set(L.F_PHI, phis)
        dev.set(L.F_OT, dev.calc_overlap())
        if nbp:
            dev.bp_configure(nbp)
        if fuse_first:
            dev.estimates_fuse_next()
        for _ in range(max(1, nbp)):
            dev.propagate(None, 0.0)
        dev.launch_trace(True)
        action(dev, model)
        dev.propagate(None, 0.0)
        trace = dev.launch_trace_get()
        dev.launch_trace(False)
        assert numpy.all(numpy.isfinite(dev.get(L.F_WEIGHT)))
        return {k: int(v[0]) for k, v in sorted(trace.items()) if OURS.search(k)}
    finally:
        dev.close()


EXPECTED = {
    'rhf64/nothing': {'(greens_tiny_kernel<true>)': 1, 'force_bias_generic_impl': 1},
    'rhf64/reortho': {'(greens_tiny_kernel<true>)': 1, 'force_bias_generic_impl': 1},
    'rhf64/comb': {'(greens_tiny_kernel<true>)': 1, 'force_bias_generic_impl': 1},
    'rhf64/set_phi': {'(greens_tiny_kernel<true>)': 2, 'force_bias_generic_impl': 1},
    'rhf64/estimates_update': {'(greens_tiny_kernel<true>)': 1, 'force_bias_generic_impl': 1},
    'rhf64/fused_nothing': {'(greens_tiny_kernel<true>)': 1, 'force_bias_generic_impl': 1},
    'rhf64/fused_local_energy': {'(greens_tiny_kernel<true>)': 2, 'force_bias_generic_impl': 1},
    'rhf64/fused_get_ghalf': {'(greens_tiny_kernel<true>)': 2, 'force_bias_generic_impl': 1},
    'rhf64/fused_reortho': {'(greens_tiny_kernel<true>)': 1, 'force_bias_generic_impl': 1},
    'rhf64/fused_comb': {'(greens_tiny_kernel<true>)': 2, 'force_bias_generic_impl': 1},
    'rhf64/fuse_next': {'(greens_tiny_kernel<true>)': 1, 'force_bias_generic_impl': 1},
    'rhf64/device_ptr': {'(greens_tiny_kernel<false>)': 1, '(greens_tiny_kernel<true>)': 1, 'force_bias_generic_impl': 1},
    'rhf64/bp_window': {'(greens_tiny_kernel<true>)': 3, 'force_bias_generic_impl': 1},
    'rhf24/nothing': {'(greens_tiny_kernel<true>)': 1, 'force_bias_generic_impl': 1},
    'rhf24/reortho': {'(greens_tiny_kernel<true>)': 1, 'force_bias_generic_impl': 1},
    'rhf24/comb': {'(greens_tiny_kernel<true>)': 1, 'force_bias_generic_impl': 1},
    'rhf24/set_phi': {'(greens_tiny_kernel<true>)': 2, 'force_bias_generic_impl': 1},
    'rhf24/estimates_update': {'(greens_tiny_kernel<true>)': 1, 'force_bias_generic_impl': 1},
    'rhf24/fused_nothing': {'(greens_tiny_kernel<true>)': 1, 'force_bias_generic_impl': 1},
    'rhf24/fused_local_energy': {'(greens_tiny_kernel<true>)': 1, 'force_bias_generic_impl': 1},
    'rhf24/fused_get_ghalf': {'(greens_tiny_kernel<true>)': 1, 'force_bias_generic_impl': 1},
    'rhf24/fused_reortho': {'(greens_tiny_kernel<true>)': 1, 'force_bias_generic_impl': 1},
    'rhf24/fused_comb': {'(greens_tiny_kernel<true>)': 1, 'force_bias_generic_impl': 1},
    'rhf24/fuse_next': {'(greens_tiny_kernel<true>)': 1, 'force_bias_generic_impl': 1},
    'rhf24/device_ptr': {'(greens_tiny_kernel<false>)': 1, '(greens_tiny_kernel<true>)': 1, 'force_bias_generic_impl': 1},
    'rhf24/bp_window': {'(greens_tiny_kernel<true>)': 3, 'force_bias_generic_impl': 1},
    'msd2/nothing': {'(greens_tiny_kernel<true>)': 2, 'force_bias_generic_impl': 2},
    'msd2/reortho': {'(greens_tiny_kernel<true>)': 4, 'force_bias_generic_impl': 2},
    'msd2/comb': {'(greens_tiny_kernel<true>)': 4, 'force_bias_generic_impl': 2},
    'msd2/set_phi': {'(greens_tiny_kernel<true>)': 4, 'force_bias_generic_impl': 2},
    'msd2/estimates_update': {'(greens_tiny_kernel<true>)': 2, 'force_bias_generic_impl': 2},
    'msd2/fused_nothing': {'(greens_tiny_kernel<true>)': 2, 'force_bias_generic_impl': 2},
    'msd2/fused_local_energy': {'(greens_tiny_kernel<true>)': 2, 'force_bias_generic_impl': 2},
    'msd2/fused_get_ghalf': {'(greens_tiny_kernel<true>)': 2, 'force_bias_generic_impl': 2},
    'msd2/fused_reortho': {'(greens_tiny_kernel<true>)': 4, 'force_bias_generic_impl': 2},
    'msd2/fused_comb': {'(greens_tiny_kernel<true>)': 4, 'force_bias_generic_impl': 2},
    'msd2/fuse_next': {'(greens_tiny_kernel<true>)': 2, 'force_bias_generic_impl': 2},
    'msd2/device_ptr': {'(greens_tiny_kernel<false>)': 2, '(greens_tiny_kernel<true>)': 2, 'force_bias_generic_impl': 2},
    'hub8x8/nothing': {'det_combine_kernel': 1, 'gj_big_kernel (fallback pass)': 1, 'gj_mfma_kernel': 1,
                       'k_greens_big: GhalfProb GEMM': 1, 'k_greens_big: OvlpProb GEMM': 1},
    'hub8x8/reortho': {'det_combine_kernel': 1, 'gj_big_kernel (fallback pass)': 1, 'gj_mfma_kernel': 1,
                       'k_greens_big: GhalfProb GEMM': 1, 'k_greens_big: OvlpProb GEMM': 1},
    'hub8x8/comb': {'det_combine_kernel': 1, 'gj_big_kernel (fallback pass)': 1, 'gj_mfma_kernel': 1,
                    'k_greens_big: GhalfProb GEMM': 1, 'k_greens_big: OvlpProb GEMM': 1},
    'hub8x8/set_phi': {'det_combine_kernel': 2, 'gj_big_kernel (fallback pass)': 2, 'gj_mfma_kernel': 2,
                       'k_greens_big: GhalfProb GEMM': 2, 'k_greens_big: OvlpProb GEMM': 2},
    'hub8x8/estimates_update': {'det_combine_kernel': 1, 'gj_big_kernel (fallback pass)': 1, 'gj_mfma_kernel': 1,
                                'k_greens_big: GhalfProb GEMM': 1, 'k_greens_big: OvlpProb GEMM': 1},
    'hub8x8/fused_nothing': {'det_combine_kernel': 1, 'gj_big_kernel (fallback pass)': 1, 'gj_mfma_kernel': 1,
                             'k_greens_big: GhalfProb GEMM': 1, 'k_greens_big: OvlpProb GEMM': 1},
    'hub8x8/fused_local_energy': {'det_combine_kernel': 2, 'gj_big_kernel (fallback pass)': 2, 'gj_mfma_kernel': 2,
                                  'k_greens_big: GhalfProb GEMM': 2, 'k_greens_big: OvlpProb GEMM': 2},
    'hub8x8/fused_get_ghalf': {'det_combine_kernel': 2, 'gj_big_kernel (fallback pass)': 2, 'gj_mfma_kernel': 2,
                               'k_greens_big: GhalfProb GEMM': 2, 'k_greens_big: OvlpProb GEMM': 2},
    'hub8x8/fused_reortho': {'det_combine_kernel': 1, 'gj_big_kernel (fallback pass)': 1, 'gj_mfma_kernel': 1,
                             'k_greens_big: GhalfProb GEMM': 1, 'k_greens_big: OvlpProb GEMM': 1},
    'hub8x8/fused_comb': {'det_combine_kernel': 2, 'gj_big_kernel (fallback pass)': 2, 'gj_mfma_kernel': 2,
                          'k_greens_big: GhalfProb GEMM': 2, 'k_greens_big: OvlpProb GEMM': 2},
    'hub8x8/fuse_next': {'det_combine_kernel': 1, 'gj_big_kernel (fallback pass)': 1, 'gj_mfma_kernel': 1,
                         'k_greens_big: GdiagProb GEMM': 1, 'k_greens_big: OvlpProb GEMM': 1},
    'hub8x8/device_ptr': {'det_combine_kernel': 2, 'gj_big_kernel (fallback pass)': 2, 'gj_mfma_kernel': 2,
                          'k_greens_big: GhalfProb GEMM': 1, 'k_greens_big: OvlpProb GEMM': 2},
}


@pytest.mark.parametrize("config,scenario", CASES, ids=["%s-%s" % cs for cs in CASES])
def test_greens_function_launches_of_a_segment(config, scenario):
    got = trace_segment(config, scenario)
    print(config, scenario, got)
    assert got == EXPECTED["%s/%s" % (config, scenario)]
