"""Generic Hamiltonians with complex Cholesky vectors on the device (afq_set_system_generic_c128): Hermitian and
general L against the CPU oracle and the genuine reference's fixtures (tests/golden/make_golden_cplx.py), through the
small-tile and work-group VHS products, the fused and the separate-GEMM propagators, NOMSD trials, back-propagation,
the driver trajectory, and the real path when the imaginary parts are zero."""
import ctypes

import numpy
import pytest

from oracle import afqmc_ref as ref
from pauxy_amd import _lib as L
from pauxy_amd import systems, trial as trial_mod
from pauxy_amd.context import release_context
from pauxy_amd.device import AfqDevice
from pauxy_amd.propagation import setup
from tests.helpers import cplx_chol, generic_model, make_device, msd_model
from tests.test_gpu_traj import replay

pytestmark = pytest.mark.gpu
TOL = 1e-10


def close(a, b, tol=TOL):
    a, b = numpy.asarray(a), numpy.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(1.0, float(numpy.max(numpy.abs(b))))
    err = float(numpy.max(numpy.abs(a - b))) / scale
    assert err <= tol, err


def build(M, K, na, nb, herm, complex_trial=True, seed=3, dt=0.01, edit=None):
    """edit: a function of the drawn Cholesky vectors [M*M, K] returning the ones the system gets."""
    rng = numpy.random.RandomState(seed)
    h = rng.normal(size=(M, M))
    h1e = 0.5 * (h + h.T) - 2.0 * numpy.eye(M)
    chol = cplx_chol(M, K, herm, rng)
    if edit is not None:
        chol = numpy.ascontiguousarray(edit(chol))
    s = systems.Generic((na, nb), numpy.array([h1e, h1e]), chol, ecore=0.37)
    e, v = numpy.linalg.eigh(h1e)
    psi = numpy.zeros((M, na + nb), dtype=complex)
    psi[:, :na] = v[:, :na]
    psi[:, na:] = v[:, :nb]
    if complex_trial:
        psi = psi + 0.05 * (rng.rand(M, na + nb) + 1j * rng.rand(M, na + nb))
    t = trial_mod.SingleDetTrial(s, psi)
    BH1, mf = setup.generic_propagator_arrays(s, t, dt)
    model = ref.RefModel('generic', M, na, nb, t.psi, BH1, mf, dt, hs_pot=s.hs_pot, rchol=t._rchol,
                         H1=s.H1.astype(complex), ecore=0.37)
    return model, rng


def walkers(model, rng, nw):
    M, ne = model.M, model.na + model.nb
    return numpy.array([model.psi + 0.1 * (rng.rand(M, ne) + 1j * rng.rand(M, ne)) for _ in range(nw)])


@pytest.mark.parametrize("herm", [True, False])
@pytest.mark.parametrize("M,K,nw", [(21, 30, 5), (37, 45, 40), (100, 60, 256), (120, 40, 40)])
def test_vhs_and_step(herm, M, K, nw):
    """VHS of both forms against the oracle (small tiles for nw <= 32, the work-group ring above), then one phaseless
    step on a few walkers (fused propagator up to M = 104, k_prop_fused_supported; separate GEMMs for M = 120)."""
    model, rng = build(M, K, 5, 4, herm)
    dev = make_device(model, nw)
    xs = rng.normal(size=(nw, K)) + 1j * rng.normal(size=(nw, K))
    vhs = dev.vhs(xs)
    close(vhs[:, 0], numpy.array([model.vhs(x) for x in xs]))
    assert abs(vhs[0, 0, 2, 7] - vhs[0, 0, 7, 2]) > 1e-6
    assert dev.kernel_issued_flops(L.K_VHS) > 0
    phis = walkers(model, rng, nw)
    dev.set(L.F_PHI, phis)
    dev.set(L.F_OT, dev.calc_overlap())
    xi = rng.normal(size=(nw, K))
    dev.propagate(xi, -1.5)
    out_phi, out_w = dev.get(L.F_PHI), dev.get(L.F_WEIGHT)
    for i in sorted({0, 1, nw // 2, nw - 1}):
        w = ref.new_walker(model, phis[i])
        ref.propagate_walker_phaseless(model, w, xi[i], -1.5)
        close(out_phi[i], w['phi'])
        close(out_w[i], w['weight'])
    dev.close()


@pytest.mark.parametrize("tag", ['H_', 'E_', 'N_'])
def test_fixture_ops(golden, tag):
    """Green's functions, force bias, VHS, exponential, half-rotated and full-G energies and (equal spins) one
    phaseless step against the genuine reference."""
    d = golden('cplx_ops.npz')
    model = generic_model(d, tag)
    na, nb = model.na, model.nb
    dev = make_device(model, 3)
    phi = d[tag + 'phi']
    dev.set(L.F_PHI, numpy.array([phi] * 3))
    det = dev.greens(want_G=True)
    close(det[0], d[tag + 'det'])
    close(dev.get(L.F_GHALF)[0], numpy.concatenate([d[tag + 'Ghalf_a'], d[tag + 'Ghalf_b']]))
    close(dev.get(L.F_G)[0], d[tag + 'G'])
    close(dev.force_bias()[0], d[tag + 'xbar'])
    xs = d[tag + 'xi'] - d[tag + 'xbar']
    vhs = dev.vhs(numpy.array([xs] * 3))
    close(vhs[0, 0], d[tag + 'VHS'])
    dev.apply_exponential(vhs)
    close(dev.get(L.F_PHI)[0], d[tag + 'phi_exp'])
    dev.set(L.F_PHI, numpy.array([phi] * 3))
    dev.greens()
    close(dev.local_energy()[0], d[tag + 'energy'])
    close(dev.local_energy_full_g(numpy.array([d[tag + 'G']]))[0], d[tag + 'energy_full'])
    if tag + 'step_phi' in d:
        dev.set(L.F_PHI, numpy.array([phi] * 3))
        dev.set(L.F_OT, dev.calc_overlap())
        dev.set(L.F_HYBRID_ENERGY, numpy.full(3, 0.25 + 0.1j))
        dev.propagate(numpy.array([d[tag + 'xi']] * 3), 0.3)
        close(dev.get(L.F_PHI)[0], d[tag + 'step_phi'])
        close(dev.get(L.F_WEIGHT)[0], d[tag + 'step_weight'])
        close(dev.get(L.F_OT)[0], d[tag + 'step_ot'])
        close(dev.get(L.F_HYBRID_ENERGY)[0], d[tag + 'step_ehyb'])
    dev.close()


@pytest.mark.parametrize("batched", [False, True])
def test_traj_cplx(golden, monkeypatch, batched):
    """The reference driver's trajectory with Hermitian complex L through AFQMC.run and run_batched."""
    d = golden('traj_cplx.npz')
    na, nb = [int(x) for x in d['nelec']]
    s = systems.Generic((na, nb), numpy.array([d['h1e'], d['h1e']]), d['chol'], float(d['ecore']),
                        h1e_mod=d['h1e_mod'])
    t = trial_mod.SingleDetTrial(s, d['psi'])
    replay(d, s, t, {}, monkeypatch, batched=batched)
    release_context(s, t)


@pytest.mark.parametrize("fb_mode", [1, 2])
def test_nomsd_hermitian(fb_mode):
    """NOMSD trial with Hermitian complex L against force_bias_msd / local_energy_msd, through the per-determinant
    contraction (mode 1) and the determinant-averaged G with its symmetric and antisymmetric parts (mode 2)."""
    rng = numpy.random.RandomState(9)
    M, K, na, nb, ndet, nw = 12, 20, 3, 2, 3, 40
    h = rng.normal(size=(M, M))
    h1e = 0.5 * (h + h.T) - 2.0 * numpy.eye(M)
    chol = cplx_chol(M, K, True, rng)
    psi = rng.normal(size=(ndet, M, na + nb)) + 1j * rng.normal(size=(ndet, M, na + nb))
    coeffs = rng.normal(size=ndet) + 1j * rng.normal(size=ndet)
    s = systems.Generic((na, nb), numpy.array([h1e, h1e]), chol, ecore=0.2)
    t = trial_mod.MultiDetTrial(s, (coeffs, psi))
    BH1, mf = setup.generic_propagator_arrays(s, t, 0.005)
    m = ref.RefModel('generic_msd', M, na, nb, psi, BH1, mf, 0.005, coeffs=coeffs, hs_pot=chol,
                     H1=numpy.array([h1e, h1e]).astype(complex), ecore=0.2)
    dev = make_device(m, nw)
    dev.set_msd_force_bias(fb_mode)
    assert dev.msd_force_bias() == fb_mode
    phis = numpy.array([psi[0] + 0.2 * (rng.rand(M, na + nb) + 1j * rng.rand(M, na + nb)) for _ in range(nw)])
    dev.set(L.F_PHI, phis)
    dev.greens()
    refs = [m.greens(p) for p in phis]
    close(dev.force_bias(), numpy.array([m.force_bias(r[1], r[2]) for r in refs]))
    close(dev.local_energy(), numpy.array([m.local_energy(r[2], r[1]) for r in refs]))
    dev.close()


@pytest.mark.parametrize("fb_mode", [1, 2])
def test_nomsd_fixture(golden, fb_mode):
    """The reference's ten NOMSD steps with Hermitian complex L (msd_cplx.npz): walker 0 replays the recorded fields,
    the others are checked against the oracle, in both force-bias modes."""
    d = golden('msd_cplx.npz')
    tag, nw = 'N_', 40
    m = msd_model(d, tag)
    dev = make_device(m, nw, hybrid=True)
    dev.set_msd_force_bias(fb_mode)
    assert dev.msd_force_bias() == fb_mode
    rng = numpy.random.RandomState(3)
    phi0 = numpy.array([d[tag + 'phi0']] + [d[tag + 'phi0'] + 0.05 * (rng.rand(m.M, m.na + m.nb) +
                                                                       1j * rng.rand(m.M, m.na + m.nb))
                                            for _ in range(nw - 1)])
    dev.set(L.F_PHI, phi0)
    ot = dev.greens()
    close(ot[0], d[tag + 'ot0'])
    refs = [m.greens(p) for p in phi0]
    xbar = dev.force_bias()
    close(xbar, numpy.array([m.force_bias(r[1], r[2]) for r in refs]))
    close(xbar[0], d[tag + 'xbar0'])
    dev.greens()
    E = dev.local_energy()
    close(E[0], d[tag + 'energy0'])
    dev.set(L.F_OT, ot)
    ws = [ref.new_walker(m, p) for p in phi0[:3]]
    eshift = complex(d[tag + 'eshift'])
    xi_rec = d[tag + 'xi']
    for i in range(xi_rec.shape[0]):
        xi = numpy.array([xi_rec[i]] + [rng.normal(size=m.nfields) for _ in range(nw - 1)])
        dev.propagate(xi, eshift)
        for w, x in zip(ws, xi):
            ref.propagate_walker_phaseless(m, w, x, eshift, hybrid=True)
        phi, wt = dev.get(L.F_PHI), dev.get(L.F_WEIGHT)
        close(phi[:3], numpy.array([w['phi'] for w in ws]), 1e-9)
        close(wt[:3], numpy.array([w['weight'] for w in ws]), 1e-9)
        close(phi[0], d[tag + 'step_phi'][i], 1e-9)
        close(wt[0], d[tag + 'step_weight'][i], 1e-9)
        close(dev.get(L.F_HYBRID_ENERGY)[0], d[tag + 'step_ehyb'][i], 1e-9)
    dev.close()


def test_vhs_issued_flops_small_tiles():
    """The small-tile VHS count against the closed form on a shape no tile choice pads (general L: 2 launches of
    nw x M^2 x K, two real MFMA products per complex-by-real pair, 2 flops each); the ring count is bounded below by
    the same work and above by its padding."""
    M, K, nw = 16, 32, 32
    model, rng = build(M, K, 3, 3, False)
    dev = make_device(model, nw)
    dev.vhs(rng.normal(size=(nw, K)) + 1j * rng.normal(size=(nw, K)))
    assert dev.kernel_issued_flops(L.K_VHS) == 2 * 4.0 * nw * M * M * K
    dev.close()
    M, K, nw = 37, 45, 40
    model, rng = build(M, K, 3, 3, True)
    dev = make_device(model, nw)
    dev.vhs(rng.normal(size=(nw, K)) + 1j * rng.normal(size=(nw, K)))
    work = 4.0 * nw * K * (M * (M + 1) // 2 + M * (M - 1) // 2)
    pad = 4.0 * 64 * 48 * (((M * (M + 1) // 2) + 159) // 160 * 160 + ((M * (M - 1) // 2) + 159) // 160 * 160)
    assert work <= dev.kernel_issued_flops(L.K_VHS) <= pad
    dev.close()


def test_back_propagation_hermitian_and_general():
    """Hermitian L: afq_bp_update against back_propagate_generic (energies from the complex full-G contraction).
    General L: refused at afq_bp_configure."""
    M, K, na, nb = 37, 45, 7, 6
    model, rng = build(M, K, na, nb, True)
    nw, nbp, nstblz = 5, 4, 3
    dev = make_device(model, nw)
    phis = walkers(model, rng, nw)
    dev.set(L.F_PHI, phis)
    dev.set(L.F_OT, dev.calc_overlap())
    dev.bp_configure(nbp)
    ws = [ref.new_walker(model, p) for p in phis]
    for w in ws:
        w['bp'] = ref.bp_new(K, nbp)
        w['phi_old'] = w['phi'].copy()
    for step in range(nbp):
        xi = rng.normal(size=(nw, K))
        dev.propagate(xi, 0.2)
        for w, x in zip(ws, xi):
            ref.propagate_walker_phaseless(model, w, x, 0.2)
    est = numpy.zeros(4 + 2 * M * M, dtype=complex)
    ref.bp_update(model, ws, nstblz, est, None, eval_energy=True)
    energies, denom, G = dev.bp_update(model.psi, nstblz, None, eval_energy=True)
    close(denom, est[3], 1e-9)
    close(G, est[4:].reshape(2, M, M), 1e-8)
    close(energies, est[:3], 1e-8)
    dev.close()
    model, rng = build(21, 30, 4, 3, False)
    dev = make_device(model, 3)
    with pytest.raises(L.AfqError) as err:
        dev.bp_configure(3)
    assert 'Hermitian' in str(err.value)
    dev.close()


def test_c3_closed_shell_walkers():
    """C3 sizes (M=100, K=500, 25+25, RHF trial, 256 walkers) with Hermitian complex L: a few steps against the
    oracle on a subset of walkers; the closed-shell forms engage (device counters)."""
    M, K, N, nw = 100, 500, 25, 256
    model, rng = build(M, K, N, N, True, complex_trial=False, seed=5, dt=0.005)
    dev = make_device(model, nw)
    phi0 = numpy.array([model.psi.copy() for _ in range(nw)])
    dev.set(L.F_PHI, phi0)
    dev.set(L.F_OT, dev.calc_overlap())
    dev.counters(reset=True, n=8)
    sub = [0, 77, 255]
    ws = [ref.new_walker(model, phi0[i]) for i in sub]
    for step in range(3):
        xi = rng.normal(size=(nw, K))
        dev.propagate(xi, -1.0)
        for w, i in zip(ws, sub):
            ref.propagate_walker_phaseless(model, w, xi[i], -1.0)
    phi, wt = dev.get(L.F_PHI), dev.get(L.F_WEIGHT)
    for w, i in zip(ws, sub):
        close(phi[i], w['phi'], 1e-9)
        close(wt[i], w['weight'], 1e-9)
    c = dev.counters(n=8)
    assert c[3] + c[7] > 0, c
    dev.close()


@pytest.mark.parametrize("M,nw,na,nb,imag", [
    pytest.param(21, 5, 4, 3, 0.0, id="21-5"), pytest.param(37, 40, 4, 3, 0.0, id="37-40"),
    pytest.param(21, 5, 4, 3, -0.0, id="negzero-21-5"), pytest.param(37, 40, 4, 3, -0.0, id="negzero-37-40"),
    pytest.param(105, 33, 4, 3, -0.0, id="negzero-105-33"),             # M = 105: the separate-GEMM propagator
    pytest.param(136, 64, 40, 40, -0.0, id="negzero-136-64-closed"),    # the large-system chain, closed-shell walkers
])
def test_real_values_as_c128_bitwise(M, nw, na, nb, imag):
    """An hs_pot with zero imaginary parts (+0.0 or -0.0) through the c128 entry point takes the real path: bitwise
    equal results."""
    from tests.test_gpu_sizes import build as build_real
    closed = na == nb
    model, rng = build_real(M, 30, na, nb, not closed)
    phis = walkers(model, rng, nw)
    if closed:
        phis[:, :, nb:] = phis[:, :, :na]                   # bitwise equal spin blocks: the closed-shell forms engage
    xi = rng.normal(size=(nw, 30))
    res = []
    for entry in ('f64', 'c128'):
        dev = AfqDevice(0)
        hs = numpy.empty(model.hs_pot.shape, dtype=numpy.complex128)
        hs.real = model.hs_pot.real
        hs.imag = imag
        assert numpy.all(numpy.signbit(hs.imag) == numpy.signbit(imag))
        rchol = numpy.ascontiguousarray(model.rchol, dtype=numpy.complex128)
        H1 = numpy.ascontiguousarray(model.H1, dtype=numpy.complex128)
        f = dev.lib.afq_set_system_generic_c128 if entry == 'c128' else dev.lib.afq_set_system_generic
        hs_arg = hs if entry == 'c128' else numpy.ascontiguousarray(model.hs_pot, dtype=numpy.float64)
        dev._ck(f(dev.h, M, 30, na, nb, hs_arg.ctypes.data_as(ctypes.c_void_p), rchol.ctypes.data_as(ctypes.c_void_p),
                  H1.ctypes.data_as(ctypes.c_void_p), 0.37))
        dev.kind, dev.M, dev.K, dev.na, dev.nb = 'generic', M, 30, na, nb
        dev.set_trial(model.psi)
        dev.set_propagator(model.BH1, model.mf_shift, model.dt)
        dev.walkers_alloc(nw)
        dev.set(L.F_PHI, phis)
        dev.set(L.F_OT, dev.calc_overlap())
        dev.counters(reset=True, n=8)
        dev.propagate(xi, -1.5)
        if closed:
            assert int(dev.counters(n=8)[7]) == nw
        dev.greens()
        res.append((dev.get(L.F_PHI), dev.get(L.F_WEIGHT), dev.local_energy()))
        dev.close()
    for a, b in zip(*res):
        assert numpy.array_equal(a, b)


def scaled_hermitian(chol, re, im):
    """Hermitian L_n = R_n + i I_n -> re R_n + i im I_n, set part by part (R stays exactly symmetric, I exactly
    antisymmetric, a zero factor gives +0.0)."""
    out = numpy.empty_like(chol)
    out.real = re * chol.real if re else 0.0
    out.imag = im * chol.imag
    return out


SCALINGS = {"re>>im": (1.0, 1e-8), "im>>re": (1e-8, 1.0), "imaginary": (0.0, 1.0)}


@pytest.mark.parametrize("M,K,na,nb,nw", [(37, 45, 7, 6, 40), (120, 40, 9, 9, 20)])
@pytest.mark.parametrize("scaling", list(SCALINGS))
def test_badly_scaled_hermitian_cholesky_vectors(M, K, na, nb, nw, scaling):
    """Hermitian L = R + i s I with s = 1e-8 and s = 1e8 (written 1e-8 R + i I: |L| stays O(1)) and purely imaginary L
    (R = 0: the Re panel is all zeros).  Green's function, force bias (complex half-rotated vectors), the two-launch VHS,
    the local energy under both exchange algorithms, one phaseless step (ring VHS and fused propagator at M = 37,
    small-tile VHS and the separate GEMMs at M = 120) and the NOMSD force bias of mode 2 (packed Re and Im contractions
    of the averaged G) against the oracle.  Pins of test_gpu_sizes.test_badly_scaled_operands_through_the_three_
    multiplication_products: 1e-13 normwise, 1e-10 componentwise on the parts within four decades of the largest."""
    from tests.test_gpu_sizes import _component_errors
    re, im = SCALINGS[scaling]
    model, rng = build(M, K, na, nb, True, edit=lambda c: scaled_hermitian(c, re, im))
    if scaling == "imaginary":
        assert numpy.all(model.hs_pot.real == 0.0) and not numpy.any(numpy.signbit(model.hs_pot.real))
    dev = make_device(model, nw)
    phis = walkers(model, rng, nw)
    dev.set(L.F_PHI, phis)
    det = dev.greens(want_G=True)
    refs = [model.greens(p) for p in phis]
    checks = {"det": _component_errors(det, numpy.array([r[0] for r in refs])),
              "G": _component_errors(dev.get(L.F_G), numpy.array([r[2] for r in refs]))}
    xbar = dev.force_bias()
    checks["xbar"] = _component_errors(xbar, numpy.array([model.force_bias(r[1], r[2]) for r in refs]))
    xs = rng.normal(size=(nw, K)) + 1j * rng.normal(size=(nw, K))
    checks["vhs"] = _component_errors(dev.vhs(xs)[:, 0], numpy.array([model.vhs(x) for x in xs]))
    want = numpy.array([model.local_energy(r[2], r[1]) for r in refs])
    for mode in (1, 2):
        dev.set_exchange_algorithm(mode)
        dev.greens()
        checks["energy%d" % mode] = _component_errors(dev.local_energy(), want)
    dev.set(L.F_PHI, phis)
    dev.set(L.F_OT, det)
    xi = rng.normal(size=(nw, K))
    dev.propagate(xi, -0.2)
    sub = sorted({0, 1, nw // 2, nw - 1})
    ws = [ref.new_walker(model, phis[i]) for i in sub]
    for w, i in zip(ws, sub):
        ref.propagate_walker_phaseless(model, w, xi[i], -0.2)
    checks["phi"] = _component_errors(dev.get(L.F_PHI)[sub], numpy.array([w['phi'] for w in ws]))
    checks["ot"] = _component_errors(dev.get(L.F_OT)[sub], numpy.array([w['ot'] for w in ws]))
    checks["weight"] = _component_errors(dev.get(L.F_WEIGHT)[sub], numpy.array([w['weight'] for w in ws]))
    dev.bp_configure(2)                                   # classified Hermitian: back-propagation is accepted
    dev.close()
    # NOMSD, averaged-G force bias with the antisymmetric fold
    ndet, nt = 3, na + nb
    dets = numpy.array([model.psi + 0.05 * (rng.rand(M, nt) + 1j * rng.rand(M, nt)) for _ in range(ndet)])
    coeffs = rng.rand(ndet) + 0.2 + 0.3j * rng.rand(ndet)
    m = ref.RefModel('generic_msd', M, na, nb, dets, model.BH1, model.mf_shift, model.dt, coeffs=coeffs,
                     hs_pot=model.hs_pot, H1=model.H1, ecore=model.ecore)
    dev = make_device(m, nw)
    dev.set_msd_force_bias(2)
    assert dev.msd_force_bias() == 2
    dev.set(L.F_PHI, phis)
    dev.greens()
    mrefs = [m.greens(p) for p in phis[sub]]
    checks["msd_xbar"] = _component_errors(dev.force_bias()[sub], numpy.array([m.force_bias(r[1], r[2]) for r in mrefs]))
    dev.close()
    print("badly scaled Hermitian L %s M=%d: " % (scaling, M) +
          "  ".join("%s %.1e/%.1e" % (k, v[0], v[1]) for k, v in checks.items()))
    for k, (norm, comp) in checks.items():
        assert norm <= 1e-13, (k, norm)
        assert comp <= 1e-10, (k, comp)


def test_one_ulp_from_hermitian_is_general():
    """Hermitian L with the imaginary part of ONE element moved by one ulp is classified general (the test is bitwise):
    every operator and one step still match the oracle (general form), back-propagation is refused, NOMSD runs mode 1."""
    from tests.test_gpu_sizes import check_operators_and_step

    def one_ulp(c):
        c = c.copy()
        r = 5 * 21 + 9                                   # L_n[5, 9], n = 3
        c[r, 3] = complex(c[r, 3].real, numpy.nextafter(c[r, 3].imag, numpy.inf))
        return c
    M, K, na, nb, nw = 21, 30, 5, 4, 40
    model, rng = build(M, K, na, nb, True, edit=one_ulp)
    Ln = model.hs_pot.reshape(M, M, K)
    assert numpy.count_nonzero(Ln != Ln.conj().transpose(1, 0, 2)) == 2
    check_operators_and_step(model, rng, nw, 'general')
    dev = make_device(model, 3)
    with pytest.raises(L.AfqError) as err:
        dev.bp_configure(3)
    assert 'Hermitian' in str(err.value)
    dev.close()
    ndet = 3
    dets = numpy.array([model.psi + 0.05 * (rng.rand(M, na + nb) + 1j * rng.rand(M, na + nb)) for _ in range(ndet)])
    coeffs = rng.rand(ndet) + 0.2 + 0.3j * rng.rand(ndet)
    m = ref.RefModel('generic_msd', M, na, nb, dets, model.BH1, model.mf_shift, model.dt, coeffs=coeffs,
                     hs_pot=model.hs_pot, H1=model.H1, ecore=model.ecore)
    dev = make_device(m, nw)
    dev.set_msd_force_bias(2)
    assert dev.msd_force_bias() == 1
    phis = walkers(model, rng, nw)
    dev.set(L.F_PHI, phis)
    dev.greens()
    close(dev.force_bias()[:4], numpy.array([m.force_bias(r[1], r[2]) for r in (m.greens(p) for p in phis[:4])]))
    dev.close()
