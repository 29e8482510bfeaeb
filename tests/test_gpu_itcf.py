"""Imaginary-time Green's function on the device (afq_itcf_configure / afq_itcf_update, k_itcf.hip): walkers
propagated on the device with fields from the test, their recorded histories replayed through the extended-precision
restatement (tests/itcf_ref_ext.py) and the device's window sums compared with it under the rule of that module (a
bound per case from the fp64 restatement's own distance to the extended one, per slice; every comparison prints its
figures); the window's lesser function at tau = 0 against the back-propagated one-body RDM of the same history; a full
AFQMC run that writes and reads back the estimator.  tests/test_gpu_itcf_shapes.py: the dispatch paths and sequences."""
import numpy
import pytest

from pauxy_amd import _lib as L, trial as trial_mod
from pauxy_amd.qmc.afqmc import AFQMC
from pauxy_amd.utils.io import extract_itcf
from tests import itcf_ref
from tests.itcf_models import compare_window, generic_model, hirsch_device, restore_factors
from tests.helpers import make_device
from tests.test_gpu_traj import close

pytestmark = pytest.mark.gpu


def check_window(case, dev, kind, model, fields, phi0, psi_T, na, nmax, nstblz, stable, wfac, **kw):
    """One afq_itcf_update against the extended restatement of the recorded histories, under the rule of
    tests/itcf_ref_ext.py (a bound from the case's own fp64-against-extended error, per slice): compare_window."""
    spgf, den = dev.itcf_update(psi_T, nstblz)
    compare_window(case, (spgf, den), kind, model, numpy.asarray(fields), phi0, psi_T, na, nmax, nstblz, stable, wfac, **kw)
    return spgf, den


def run_generic(M, K, na, nb, nw, nmax, neqlb, nstblz, stable, restore, dead=(), seed=3, hermitian=False):
    model, s, rng = generic_model(M, K, na, nb, seed, hermitian=hermitian)
    dev = make_device(model, nw)
    ne = na + nb
    dev.set(L.F_PHI, numpy.array([model.psi + 0.1 * (rng.rand(M, ne) + 1j * rng.rand(M, ne)) for _ in range(nw)]))
    dev.set(L.F_OT, dev.calc_overlap())
    if dead:
        w = dev.get(L.F_WEIGHT).copy()
        w[list(dead)] = 0.0
        dev.set(L.F_WEIGHT, w)
    dev.itcf_configure(nmax, neqlb, stable, restore)
    phi0 = dev.get(L.F_PHI).copy()
    xs = []
    for step in range(nmax + neqlb):
        dev.propagate(rng.normal(size=(nw, K)), 0.2)
        xs.append(dev.get(L.F_XSHIFTED).copy())
    xs = numpy.array(xs)
    wfac = restore_factors(dev, model.psi, nstblz) if restore else dev.get(L.F_WEIGHT).astype(complex)
    for d in dead:
        assert wfac[d] == 0
    case = "generic%s M=%d %d+%d nw=%d nmax=%d neqlb=%d nstblz=%d %s%s" % (
        ' (H)' if hermitian else '', M, na, nb, nw, nmax, neqlb, nstblz, 'stable' if stable else 'unstable',
        ' restore' if restore else '')
    out = check_window(case, dev, 'generic', (numpy.asarray(s.hs_pot), numpy.asarray(model.BH1), model.dt), xs, phi0,
                       model.psi, na, nmax, nstblz, stable, wfac)
    dev.close()
    return out


@pytest.mark.parametrize("M,K,na,nb,nw,nmax,neqlb,nstblz,stable,restore,dead", [
    (16, 24, 5, 3, 1, 4, 0, 5, True, False, ()),
    (16, 24, 5, 3, 37, 7, 2, 3, True, False, (4,)),
    (16, 24, 5, 3, 37, 7, 2, 3, False, False, (4,)),
    (16, 24, 5, 3, 256, 6, 3, 4, True, False, (0, 200)),
    (16, 24, 5, 3, 5, 6, 1, 2, True, True, (1,)),
    (16, 24, 5, 3, 5, 6, 1, 2, False, True, ()),
    (64, 80, 11, 8, 4, 5, 2, 3, True, False, ()),
    (100, 120, 13, 9, 3, 6, 1, 4, True, False, (2,)),
    (100, 120, 13, 9, 3, 6, 1, 4, False, True, ()),
])
def test_generic_window_against_restatement(M, K, na, nb, nw, nmax, neqlb, nstblz, stable, restore, dead):
    run_generic(M, K, na, nb, nw, nmax, neqlb, nstblz, stable, restore, dead)


@pytest.mark.parametrize("M,nw,stable,restore", [(16, 9, True, False), (16, 9, False, True), (64, 4, True, True)])
def test_hermitian_complex_vectors(M, nw, stable, restore):
    """Hermitian complex L_n: the complex VHS builder feeds the B matrices, B(-conj(x)) is still B(x)^H."""
    model, s, rng = generic_model(M, 20, 5, 3, hermitian=True)
    assert numpy.iscomplexobj(s.hs_pot) and numpy.any(numpy.asarray(s.hs_pot).imag != 0)
    run_generic(M, 20, 5, 3, nw, 5, 2, 3, stable, restore, (1,), hermitian=True)


def test_stable_and_unstable_windows_agree():
    a, da = run_generic(16, 24, 5, 3, 7, 8, 0, 3, True, False)
    b, db = run_generic(16, 24, 5, 3, 7, 8, 0, 3, False, False)
    assert da == db
    print("ITCF-PAIR | stable vs unstable M=16 nw=7 nmax=8 | %.2e" % (numpy.max(numpy.abs(a - b)) / max(1.0, numpy.max(numpy.abs(b)))))
    close(a, b, 2e-13)            # each is within bound(err_ref) of the extended restatement (1e-13 here: ITCF-CASE lines)


@pytest.mark.parametrize("nx,na,nb,nw,nmax,neqlb,nstblz,stable", [
    (4, 7, 5, 1, 5, 0, 2, True),
    (4, 7, 5, 37, 6, 2, 4, True),
    (4, 7, 5, 37, 6, 2, 4, False),
    (4, 7, 7, 256, 4, 1, 2, True),
    (8, 30, 26, 5, 5, 2, 3, True),
])
def test_hirsch_window_against_restatement(nx, na, nb, nw, nmax, neqlb, nstblz, stable):
    dev, BT2, psi, rng, U, dt = hirsch_device(nx, nx, na, nb, nw)
    M = nx * nx
    dev.itcf_configure(nmax, neqlb, stable, False)
    phi0 = dev.get(L.F_PHI).copy()
    fields = []
    for step in range(nmax + neqlb):
        dev.hirsch_kinetic()
        f, _ = dev.hirsch_two_body(rng.random_sample((nw, M)))
        dev.hirsch_finish(0.0)
        fields.append(f)
    fields = numpy.array(fields)
    wfac = dev.get(L.F_WEIGHT).astype(complex)
    wfac[(fields < 0).any(axis=(0, 2))] = 0.0          # a walker that died inside the window has no complete history
    case = "hirsch %dx%d %d+%d nw=%d nmax=%d neqlb=%d nstblz=%d %s" % (nx, nx, na, nb, nw, nmax, neqlb, nstblz,
                                                                      'stable' if stable else 'unstable')
    check_window(case, dev, 'hirsch', (BT2, dt, U), fields, phi0, psi, na, nmax, nstblz, stable, wfac)
    dev.close()


def test_lesser_function_at_zero_is_the_back_propagated_rdm():
    """Gls(0) = P(0) = gab(psi_L(0), psi_R(0)) is the back-propagated G of the same window, whose device sum holds the
    transpose (G_bp = gab(phi_bp, phi_old)^T, back_propagation.py:156-157)."""
    model, s, rng = generic_model(16, 24, 5, 3)
    nw, n = 9, 6
    dev = make_device(model, nw)
    dev.set(L.F_PHI, numpy.array([model.psi + 0.1 * rng.rand(16, 8) for _ in range(nw)]))
    dev.set(L.F_OT, dev.calc_overlap())
    dev.itcf_configure(4, n - 4, True, False)
    for step in range(n):
        dev.propagate(rng.normal(size=(nw, 24)), 0.2)
    _, den_bp, G_bp = dev.bp_update(model.psi, 3, None, reset=False)
    spgf, den = dev.itcf_update(model.psi, 3)
    close(den, den_bp, 1e-12)
    want = G_bp.transpose(0, 2, 1).real
    print("ITCF-PAIR | Gls(0) vs back-propagated RDM M=16 nw=9 | %.2e" % (numpy.max(numpy.abs(spgf[0, :, 1] - want)) / max(1.0, numpy.max(numpy.abs(want)))))
    close(spgf[0, :, 1], want, 1e-13)     # the same kernels on the same history: the order of the rule at this shape
    dev.close()


def test_history_of_another_length_is_refused():
    model, s, rng = generic_model(16, 24, 5, 3)
    dev = make_device(model, 2)
    dev.bp_configure(3)
    with pytest.raises(L.AfqError) as e:
        dev.itcf_configure(2, 2)
    assert e.value.code == -2
    dev.itcf_configure(2, 1)
    dev.close()


@pytest.mark.parametrize("mode", ['full', 'diagonal', [[0, 0], [1, 2], [3, 1]]])
def test_driver_writes_and_reads_back(tmp_path, mode):
    model, s, rng = generic_model(12, 16, 4, 3)
    t = trial_mod.SingleDetTrial(s, model.psi)
    dt = 0.01
    options = {'qmc': {'timestep': dt, 'num_steps': 4, 'blocks': 2, 'stabilise_freq': 2, 'pop_control_freq': 2,
                       'num_walkers': 6, 'rng_seed': 7},
               'estimators': {'basename': str(tmp_path / 'estimates'),
                              'itcf': {'tau_max': 2.5 * dt, 'tau_eqlb': 2.5 * dt, 'mode': mode,
                                       'restore_weights': False}}}
    afqmc = AFQMC(options=options, system=s, trial=t)
    est = afqmc.estimators.estimators['itcf']
    assert (est.nmax, est.neqlb, est.nprop_tot) == (2, 2, 4)
    afqmc.run(verbose=False)
    afqmc.finalise(verbose=False)
    assert len(est.windows) == 2
    M, na, nb = 12, 4, 3
    for g in est.windows:
        assert g.shape == (3, 2, 2, M, M) and numpy.isfinite(g).all()
        close(g[0, :, 0] + g[0, :, 1], numpy.array([numpy.eye(M)] * 2), 1e-10)
        close(numpy.trace(g[0, 0, 0]).real, M - na, 1e-10)
        close(numpy.trace(g[0, 1, 0]).real, M - nb, 1e-10)
    got = extract_itcf(str(tmp_path / 'estimates.0.h5'))
    want = numpy.array([itcf_ref.select(g, mode) for g in est.windows])
    assert got.shape == want.shape
    assert numpy.array_equal(got, want)
