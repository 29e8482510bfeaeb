"""Every operator and one full step against the oracle on shapes that sit on the kernels' dispatch boundaries: 33..45
electrons per spin (LDS Gauss-Jordan, GEMM-chain propagator), M just above / at the limits of the fused kernels (104, 105,
128, 130, 200), unequal spins, real and complex trials, populations above and below the work-group-tiled GEMM threshold."""
import pytest

from tests.helpers import lform_params
from tests.test_gpu_sizes import build, check_operators_and_step

pytestmark = pytest.mark.gpu
LFORMS = ["real", "hermitian", "general"]


def run_shape(M, K, na, nb, nw, cplx, lform='real'):
    """cplx selects a complex trial; lform the Cholesky vectors (real symmetric, Hermitian or general complex)."""
    model, rng = build(M, K, na, nb, cplx, lform=lform)
    check_operators_and_step(model, rng, nw, lform)


@pytest.mark.parametrize("M,K,na,nb,nw,cplx,lform", lform_params([
    (64, 20, 40, 37, 70, False), (100, 30, 45, 33, 66, True), (130, 16, 20, 20, 70, False), (48, 10, 33, 33, 8, False),
    (200, 12, 10, 9, 65, True), (128, 8, 32, 32, 64, False), (104, 9, 32, 31, 64, False), (105, 9, 26, 25, 64, True),
    # packed Re / Im column counts of Hermitian L (171 / 153, 190 / 171) on either side of the 160-column ring tile,
    # populations on the 32-walker switch between the small-tile and the ring VHS
    (18, 5, 4, 3, 33, True), (19, 4, 3, 3, 32, False),
], LFORMS))
def test_operators_and_step_on_boundary_shapes(M, K, na, nb, nw, cplx, lform):
    run_shape(M, K, na, nb, nw, cplx, lform)


@pytest.mark.parametrize("M,K,na,nb,nw,cplx,lform", lform_params([
    (2, 1, 1, 1, 1, False), (3, 2, 2, 1, 2, True), (4, 2, 4, 3, 5, False), (6, 3, 2, 0, 7, False), (5, 3, 1, 1, 257, True),
    (20, 10, 3, 2, 600, False), (16, 5, 16, 15, 64, False), (33, 4, 1, 0, 64, True), (17, 1, 8, 8, 63, False),
], LFORMS))
def test_operators_and_step_on_degenerate_shapes(M, K, na, nb, nw, cplx, lform):
    """The other end: two orbitals, one field, one walker; a filled band (na = M); no beta electrons; populations that are
    not a multiple of any tile (257, 600)."""
    run_shape(M, K, na, nb, nw, cplx, lform)


@pytest.mark.parametrize("nx,ny,na,nb,nw,spin", [
    (7, 7, 24, 23, 66, False), (10, 10, 45, 45, 64, False), (9, 9, 40, 38, 65, True), (6, 6, 18, 18, 70, False),
    (10, 8, 46, 45, 64, False), (12, 11, 66, 66, 9, False), (2, 2, 2, 2, 5, False), (8, 1, 4, 4, 64, True),
    (3, 3, 5, 4, 33, False), (4, 2, 3, 1, 65, True),
])
def test_hubbard_continuous_on_boundary_shapes(nx, ny, na, nb, nw, spin):
    """Hubbard, continuous fields: lattices whose electron counts straddle the 32 / 45 limits of the small Green's function
    kernel and its LDS budget, odd site counts, charge and spin decomposition, populations around 64."""
    from oracle import afqmc_ref as ref
    from pauxy_amd import systems, trial as trial_mod
    from pauxy_amd.propagation import setup
    from tests.test_gpu_fullsize import run_fullsize
    s = systems.Hubbard(nx, ny, na, nb, 4.0)
    t = trial_mod.uhf_trial_hubbard(s, ueff=0.4)
    dt = 0.01
    BH1, mf = setup.hubbard_propagator_arrays(s, t, dt, not spin)
    model = ref.RefModel('hubbard_spin' if spin else 'hubbard', nx * ny, na, nb, t.psi, BH1, mf, dt, U=4.0,
                         H1=s.T.astype(complex))
    run_fullsize(model, nw, [0, 1, nw // 2, nw - 1])


@pytest.mark.parametrize("nx,ny,na,nb,charge,nw", [
    (2, 2, 2, 2, False, 4), (8, 1, 4, 4, False, 5), (3, 3, 5, 4, False, 7), (4, 2, 3, 1, True, 4), (6, 6, 18, 17, True, 9),
    (9, 9, 40, 33, False, 4), (12, 12, 72, 70, False, 3),
])
def test_hirsch_on_small_and_odd_lattices(nx, ny, na, nb, charge, nw):
    """Discrete Hirsch fields on a 2 x 2 plaquette, a chain, odd site counts, unequal spins (either side of the 32 / 45 /
    68 electron limits of its kernels), spin and charge decomposition, a few walkers."""
    from tests.test_gpu_fullsize import run_hirsch_lattice
    run_hirsch_lattice(nx, ny, na, nb, charge, nw)


_NOMSD_ROWS = [
    (24, 10, 5, 4, 2, 9, False), (100, 30, 25, 25, 7, 64, False), (64, 12, 40, 37, 3, 20, False),
    (130, 8, 20, 19, 2, 33, False), (37, 9, 7, 6, 16, 65, False), (16, 4, 3, 0, 2, 5, False), (48, 6, 33, 33, 2, 8, False),
    # the first shape on the M > 64 templates of the averaged-G folds; a determinant with coefficient exactly 0 (its slice
    # of the averaged G is zeroed, msd_scale_ghalf_kernel) there and on the M <= 64 templates
    (65, 10, 20, 19, 3, 40, True), (24, 10, 5, 4, 3, 33, True),
]


@pytest.mark.parametrize("M,K,na,nb,ndet,nw,zero_coeff,lform", lform_params(
    _NOMSD_ROWS, LFORMS, {r: "-".join(str(x) for x in r[:6]) + ("-zero-coeff" if r[6] else "") for r in _NOMSD_ROWS}))
def test_distinct_complex_determinants_on_boundary_shapes(M, K, na, nb, ndet, nw, zero_coeff, lform):
    """NOMSD trials of 2..16 distinct complex determinants (walkers/multi_det.py:27-77, propagation/generic.py:154-157,
    estimators/mixed.py:439-448) on the dispatch boundaries of the single-determinant kernels they reuse: determinant
    weights, total overlap, weighted force bias and energy per walker against the oracle, both exchange algorithms.
    Complex L: Hermitian vectors take the averaged-G force bias with its antisymmetric fold and imaginary contraction
    (mode 2), general ones always the per-determinant contraction (mode 1)."""
    import numpy
    from oracle import afqmc_ref as ref
    from pauxy_amd import _lib as L
    from pauxy_amd import trial as trial_mod
    from pauxy_amd.device import AfqDevice
    from pauxy_amd.propagation import setup
    from tests.test_gpu_sizes import generic_system
    from tests.test_gpu_traj import close
    dt = 0.005
    s = generic_system(M, K, (na, nb), 7, lform)
    t0 = trial_mod.rhf_trial_generic(s)
    rng = numpy.random.RandomState(3)
    nt = na + nb
    dets = numpy.array([t0.psi + (0.0 if d == 0 else 0.05) * (rng.rand(M, nt) + 1j * rng.rand(M, nt)) for d in range(ndet)])
    coeffs = (rng.rand(ndet) + 0.2) * numpy.exp(1j * rng.rand(ndet))
    if zero_coeff:
        coeffs[1] = 0.0
    t = trial_mod.MultiDetTrial(s, (coeffs, dets), init=t0.psi)
    BH1, mf = setup.generic_propagator_arrays(s, t, dt)
    phis = t0.psi[None] + 0.05 * (rng.rand(nw, M, nt) + 1j * rng.rand(nw, M, nt))
    per = M * nt
    E = {}
    for mode in (1, 2):
        dev = AfqDevice(0)
        dev.set_exchange_algorithm(mode)
        dev.set_system_generic(s.hs_pot, t._rchol[:per], s.H1.astype(complex), s.ecore, na, nb)
        dev.set_trial_multi(dets, coeffs, t._rchol)
        dev.set_propagator(BH1, mf, dt)
        dev.walkers_alloc(nw)
        dev.set(L.F_PHI, phis)
        tot = dev.greens()
        wts = dev.det_weights()
        xbar = dev.force_bias()
        # both force-bias algorithms (afq_set_msd_force_bias): one contraction per determinant, and the reference's own
        # formulation through the determinant-averaged Green's function
        xb = {}
        for fbm in (1, 2):
            dev.set_msd_force_bias(fbm)
            dev.launch_trace(True)
            # (general complex L has no packed form: the averaged G is not taken, whatever the mode asks for)
            assert dev.msd_force_bias() == (1 if lform == 'general' else fbm)
            xb[fbm] = dev.force_bias()
            names = set(dev.launch_trace_get())
            dev.launch_trace(False)
            gbar = fbm == 2 and lform != 'general'
            assert ('msd_gbar_fold GEMM' in names) == gbar, names
            assert ('msd_gbar_fold_anti GEMM' in names) == (gbar and lform == 'hermitian'), names
            assert ('msd_gbar_contract_im GEMM' in names) == (gbar and lform == 'hermitian'), names
            if not gbar:
                assert not any(n.startswith('msd_gbar') for n in names), names
        close(xb[1], xb[2], 1e-11)
        close(xbar, xb[2], 1e-11)
        dev.set_msd_force_bias(0)
        dev.greens()
        E[mode] = dev.local_energy()
        dev.close()
    close(E[1], E[2], 1e-11)
    H1 = s.H1.astype(complex)
    for w in sorted({0, nw // 2, nw - 1}):
        ws, Es, Gsum = [], [], 0.0
        for d in range(ndet):
            ov, gh, G = ref.greens_function(phis[w], dets[d], na, nb)
            ws.append(numpy.conj(coeffs[d]) * ov)
            Es.append(numpy.array(ref.local_energy_generic_cholesky_opt(H1, s.ecore, G, gh, t._rchol[d * per:(d + 1) * per],
                                                                        na, nb)))
            Gsum = Gsum + ws[-1] * (G[0] + G[1])
        ws = numpy.array(ws)
        close(wts[w], ws, 1e-10)
        close(tot[w], ws.sum(), 1e-10)
        close(E[2][w], (ws[:, None] * numpy.array(Es)).sum(0) / ws.sum(), 1e-10)
        vbias = s.hs_pot.T.dot((Gsum / ws.sum()).ravel())
        close(xbar[w], -dt ** 0.5 * (1j * vbias - mf), 1e-10)
    # one full step (hybrid weights, phaseless constraint, some walkers dead) against the oracle's multi-determinant walker
    from tests.helpers import make_device
    model = ref.RefModel('generic_msd', M, na, nb, dets, BH1, mf, dt, coeffs=coeffs, hs_pot=s.hs_pot,
                         H1=numpy.array([s.H1[0], s.H1[1]]).astype(complex), ecore=s.ecore)
    dev = make_device(model, nw)
    dev.set(L.F_PHI, phis)
    w0 = numpy.ones(nw)
    w0[1::4] = 0.0
    dev.set(L.F_WEIGHT, w0)
    dev.set(L.F_OT, tot)
    xi = rng.normal(size=(nw, K))
    dev.propagate(xi, -0.7)
    out_phi, out_w, out_ot = dev.get(L.F_PHI), dev.get(L.F_WEIGHT), dev.get(L.F_OT)
    dev.close()
    for w in sorted({0, 1, nw // 2, nw - 1}):
        if w0[w] == 0.0:
            assert numpy.array_equal(out_phi[w], phis[w]) and out_w[w] == 0.0
            continue
        wk = ref.new_walker(model, phis[w])
        ref.propagate_walker_phaseless(model, wk, xi[w], -0.7)
        close(out_phi[w], wk['phi'], 1e-9)
        close(out_w[w], wk['weight'], 1e-9)
        close(out_ot[w], wk['ot'], 1e-9)


@pytest.mark.parametrize("variant", ["local_energy", "free_projection", "order4", "order9", "no_force_bias"])
@pytest.mark.parametrize("M,K,na,nb,nw,cplx", [
    (100, 30, 25, 25, 64, False), (64, 20, 40, 37, 20, True), (130, 16, 20, 20, 33, False), (37, 9, 7, 6, 65, True),
    (20, 8, 3, 0, 9, False),
])
def test_propagator_options_on_boundary_shapes(M, K, na, nb, nw, cplx, variant):
    """The other propagator options (continuous.py:30-33,82-111,175-200,264-300) on shapes of every dispatch path: local-energy
    weights, free projection, Taylor orders 4 and 9, no force bias -- one step against the oracle."""
    import numpy
    from oracle import afqmc_ref as ref
    from pauxy_amd import _lib as L
    from tests.helpers import make_device
    from tests.test_gpu_sizes import build
    from tests.test_gpu_traj import close
    model, rng = build(M, K, na, nb, cplx)
    kw = {}
    if variant == "local_energy":
        kw['hybrid'] = False
    elif variant == "free_projection":
        kw['free_projection'] = True
        kw['force_bias'] = False
    elif variant == "no_force_bias":
        kw['force_bias'] = False
    elif variant.startswith("order"):
        model.exp_order = int(variant[5:])
    dev = make_device(model, nw, **kw)
    phis = numpy.array([model.psi + 0.1 * (rng.rand(M, na + nb) + 1j * rng.rand(M, na + nb)) for _ in range(nw)])
    dev.set(L.F_PHI, phis)
    w0 = numpy.ones(nw)
    w0[2::5] = 0.0
    dev.set(L.F_WEIGHT, w0)
    dev.set(L.F_OT, dev.calc_overlap())
    xi = rng.normal(size=(nw, K))
    dev.propagate(xi, -1.1)
    out = {f: dev.get(getattr(L, 'F_' + f)) for f in ('PHI', 'WEIGHT', 'OT', 'PHASE', 'HYBRID_ENERGY')}
    dev.close()
    for w in sorted({0, 1, 2, nw // 2, nw - 1}):
        if w0[w] == 0.0:
            assert numpy.array_equal(out['PHI'][w], phis[w]) and out['WEIGHT'][w] == 0.0
            continue
        wk = ref.new_walker(model, phis[w])
        if variant == "free_projection":
            ref.propagate_walker_free(model, wk, xi[w], -1.1)
        elif variant == "no_force_bias":
            fb = model.force_bias
            model.force_bias = lambda Ghalf, G: numpy.zeros(K, dtype=complex)
            try:
                ref.propagate_walker_phaseless(model, wk, xi[w], -1.1)
            finally:
                model.force_bias = fb
        else:
            ref.propagate_walker_phaseless(model, wk, xi[w], -1.1, hybrid=(variant != "local_energy"))
        close(out['PHI'][w], wk['phi'], 1e-9)
        close(out['WEIGHT'][w], wk['weight'], 1e-9)
        close(out['OT'][w], wk['ot'], 1e-9)
        close(out['PHASE'][w], wk['phase'], 1e-9)
        if variant not in ("free_projection", "local_energy"):
            close(out['HYBRID_ENERGY'][w], wk['hybrid_energy'], 1e-9)


@pytest.mark.parametrize("rs,nup,ndown,ecut,nw", [
    (1.0, 1, 1, 1.0, 5), (3.0, 7, 7, 2.0, 65), (2.0, 19, 19, 3.0, 64), (2.0, 7, 1, 2.5, 66), (0.5, 2, 2, 6.0, 33),
    (2.0, 7, 7, 1.0, 256),
])
def test_ueg_on_other_densities_and_cutoffs(rs, nup, ndown, ecut, nw):
    """Electron gas away from BASELINE configs[1]: one electron per spin, a spin-polarised gas, 19 + 19 electrons (more
    columns than the fused plane-wave propagator takes), 179 plane waves (more rows than it takes), a 19-plane-wave basis."""
    import numpy
    from oracle import afqmc_ref as ref
    from pauxy_amd import systems, trial as trial_mod
    from pauxy_amd.propagation import setup
    from tests.test_gpu_fullsize import run_fullsize
    s = systems.UEG(rs, nup, ndown, ecut)
    t = trial_mod.hartree_fock_ueg(s)
    dt = 0.005
    BH1, mf = setup.ueg_propagator_arrays(s, t, dt)
    H1diag = numpy.array([numpy.diag(s.H1[0]), numpy.diag(s.H1[1])])
    model = ref.RefModel('ueg', s.nbasis, nup, ndown, t.psi, BH1, mf, dt, iA=s.iA, iB=s.iB, H1diag=H1diag,
                         vqvec=s.vqvec, vol=s.vol, ikpq_i=s.ikpq_i, ikpq_kpq=s.ikpq_kpq, ipmq_i=s.ipmq_i,
                         ipmq_pmq=s.ipmq_pmq, ecore=s.ecore)
    run_fullsize(model, nw, sorted({0, 2, nw // 2, nw - 1}))


@pytest.mark.parametrize("K,nw,lform", lform_params([(1, 1), (255, 33), (256, 65), (257, 31), (513, 64), (2, 129)],
                                                    ["real", "hermitian"]))
def test_field_counts_and_populations_on_kernel_boundaries(K, nw, lform):
    """Field counts around the work-group size of the fields kernel (a thread per field up to 256, a Philox pair per thread
    above), one field, populations around the 32 / 64-walker thresholds of the work-group-tiled GEMMs and a single walker."""
    run_shape(20, K, 4, 3, nw, K % 2 == 1, lform)


@pytest.mark.parametrize("nw", [2, 3, 63, 64, 65, 257, 1000, 4096])
@pytest.mark.parametrize("spread", [0.3, 2.0, "zeros"])
def test_comb_on_random_populations(nw, spread):
    """walkers/handler.py:225-338 on one rank for populations from 2 to 4096 walkers and weight distributions from narrow to
    very wide (a third of the walkers dead): parent_ix exact against the oracle's comb, the (clone, kill) pairs applied the
    reference's way (handler.py:295-301: ``zip`` truncates), every weight 1 afterwards, total weight returned."""
    import numpy
    from oracle import afqmc_ref as ref
    from pauxy_amd import _lib as L
    from tests.helpers import make_device
    from tests.test_gpu_sizes import build
    M, K, na, nb = 8, 3, 2, 2
    model, rng = build(M, K, na, nb, False)
    rs = numpy.random.RandomState(nw)
    dev = make_device(model, nw)
    phis = model.psi[None] + 0.1 * (rs.rand(nw, M, na + nb) + 1j * rs.rand(nw, M, na + nb))
    wts = numpy.exp((0.8 if spread == "zeros" else spread) * rs.normal(size=nw))
    if spread == "zeros":
        wts[rs.rand(nw) < 0.33] = 0.0
        wts[0] = max(wts[0], 0.5)
    dev.set(L.F_PHI, phis)
    dev.set(L.F_WEIGHT, wts)
    r = float(rs.rand())
    pix, tw = dev.popcontrol_comb(r, nw)
    scale = sum(wts) / nw
    want = ref.comb_parent_ix(wts / scale, nw, r)
    assert numpy.array_equal(pix, want)
    assert abs(tw - sum(wts)) <= 1e-12 * sum(wts)
    expect = phis.copy()
    for c, k in ref.comb_pairs(want):
        expect[k] = phis[c]
    assert numpy.array_equal(dev.get(L.F_PHI), expect)
    assert numpy.all(dev.get(L.F_WEIGHT) == 1.0)
    dev.close()


def _generic_40():
    from pauxy_amd import systems, trial as trial_mod
    from tests.test_gpu_batched import build_afqmc
    s = systems.synthetic_generic(64, 12, (40, 40), seed=5)
    return build_afqmc(s, trial_mod.rhf_trial_generic(s), 66)


def _generic_m130():
    from pauxy_amd import systems, trial as trial_mod
    from tests.test_gpu_batched import build_afqmc
    s = systems.synthetic_generic(130, 10, (20, 20), seed=6)
    return build_afqmc(s, trial_mod.rhf_trial_generic(s), 65)


def _generic_40_hermitian():
    from pauxy_amd import trial as trial_mod
    from tests.test_gpu_batched import build_afqmc
    from tests.test_gpu_sizes import generic_system
    s = generic_system(64, 12, (40, 40), 5, 'hermitian')
    return build_afqmc(s, trial_mod.rhf_trial_generic(s), 66)


def _generic_m130_general():
    from pauxy_amd import trial as trial_mod
    from tests.test_gpu_batched import build_afqmc
    from tests.test_gpu_sizes import generic_system
    s = generic_system(130, 10, (20, 20), 6, 'general')
    return build_afqmc(s, trial_mod.rhf_trial_generic(s), 65)


def _hubbard_10x10():
    from pauxy_amd import systems, trial as trial_mod
    from tests.test_gpu_batched import build_afqmc
    s = systems.Hubbard(10, 10, 45, 45, 4.0)
    return build_afqmc(s, trial_mod.uhf_trial_hubbard(s, ueff=0.4), 64, False, {'hubbard_stratonovich': 'continuous'})


@pytest.mark.parametrize("make", [_generic_40, _generic_m130, _hubbard_10x10, _generic_40_hermitian, _generic_m130_general],
                         ids=["generic-40e", "generic-M130", "hubbard-10x10-45e", "generic-40e-hermitian-L",
                              "generic-M130-general-L"])
def test_driver_loops_agree_on_boundary_shapes(make):
    """20 steps of the per-walker loop, the batched loop and the batched loop with the estimator terms riding on the weight
    update (which also announces the steps whose per-spin Ghalf is not stored) on shapes that take the dispatch paths
    between the benchmark configurations: same walkers, weights and block rows to rounding, identical comb decisions."""
    import numpy
    from tests.test_gpu_batched import run_c3, close
    a, blocks_a, phi_a = run_c3(False, True, make=make)
    b, blocks_b, phi_b = run_c3(True, True, make=make)
    d, blocks_d, phi_d = run_c3(True, False, ride=True, make=make)
    assert numpy.all(numpy.isfinite(phi_a.view(float))) and numpy.all(numpy.isfinite(a['weight']))
    assert numpy.array_equal(a['pix'], b['pix'])
    for other, blocks, phi in ((b, blocks_b, phi_b), (d, blocks_d, phi_d)):
        for key in ('weight', 'ot', 'ehyb'):
            close(other[key], a[key], 1e-9)
        close(phi, phi_a, 1e-9)
        close(blocks[:, 1:10], blocks_a[:, 1:10], 1e-9)
