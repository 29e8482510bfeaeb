"""Back-propagated density and spin correlation functions on the device (k_corr.hip): the kernel against the numpy
restatement (tests/corr_ref.py, itself checked against the Fock space in test_corr_cpu.py) on every tile boundary it
has, the window's weighted sums against per-walker G_bp put through the restatement on all three systems, both driver
loops on the reference's Hubbard trajectory (where U sum_i <n_i,up n_i,down> must be the window's E2b), refusals, and
bitwise reproducibility.

Tolerance: `close` of tests/test_gpu_traj.py at 1e-8 (error relative to max(1, max|want|)), the bound
test_gpu_bp_obs.py and test_gpu_ueg_sf.py use for sums of this kind."""
import numpy
import pytest

from pauxy_amd import _lib as L, systems
from pauxy_amd.device import AfqDevice, _p
from pauxy_amd.utils.io import extract_rdm
from tests import corr_ref
from tests.helpers import make_device
from tests.itcf_models import hirsch_device
from tests.test_gpu_bp_obs import build, capture_bp
from tests.test_gpu_traj import close, run_hirsch
from tests.test_gpu_ueg_sf import ListSystem, rand_G, ueg_device, ueg_model_of

pytestmark = pytest.mark.gpu
TOL = 1e-8
T = 32              # tile edge of corr_tile_kernel (CT)
WCH = 32            # walkers per chunk of the weighted sum (CORR_WCH)


# ---------------------------------------------------------------- 1. the kernel
def system_only_device(kind, M):
    """A handle that holds a system of M orbitals and nothing else: afq_correlations_full_g needs only M."""
    if kind == 'ueg':
        s = ListSystem(M, 8, M, seed=M)
        s.nup = s.ndown = 1                       # (M = 1 holds one electron per spin)
        return ueg_device(s)
    dev = AfqDevice(0)
    if kind == 'hubbard':
        dev.set_system_hubbard(numpy.zeros((2, M, M)), 4.0, 1, 1)
    else:
        K = 2
        dev.set_system_generic(numpy.zeros((M * M, K)), numpy.zeros((2 * M, K), dtype=complex),
                               numpy.zeros((2, M, M)), 0.0, 1, 1)
    return dev


_want = {}


def kernel_case(M, n):
    """Random complex G (not idempotent: nothing cancels) and its restatement, computed once per shape."""
    if (M, n) not in _want:
        G = rand_G(n, M, 31 + M + n)
        want = numpy.array([corr_ref.corr(g) for g in G])
        G.setflags(write=False)
        want.setflags(write=False)
        _want[(M, n)] = (G, want)
    return _want[(M, n)]


@pytest.mark.parametrize("kind", ['generic', 'hubbard', 'ueg'])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("M", [1, T - 1, T, T + 1, 2 * T + 1, 100, 130, 256])
def test_kernel_on_every_tile_boundary(M, n, kind):
    G, want = kernel_case(M, n)
    dev = system_only_device(kind, M)
    try:
        got = dev.correlations_full_g(G)
        again = dev.correlations_full_g(G)
    finally:
        dev.close()
    assert got.shape == (n, 5, M, M)
    err = numpy.max(numpy.abs(got - want)) / max(1.0, numpy.max(numpy.abs(want)))
    print("CORR-KERNEL | %s M=%d n=%d | rel err %.2e" % (kind, M, n, err))
    close(got, want, TOL)
    assert numpy.array_equal(got, again)                    # same input, same bits


# ---------------------------------------------------------------- 2. the window
def generic_population(nw, nbp, seed=5):
    model, h1e, Lv, rng = build(12, 8, 2, 2, seed)
    M, ne, K = 12, 4, 8
    dev = make_device(model, nw)
    dev.set(L.F_PHI, numpy.array([model.psi + 0.1 * (rng.rand(M, ne) + 1j * rng.rand(M, ne)) for _ in range(nw)]))
    dev.set(L.F_OT, dev.calc_overlap())
    dev.bp_configure(nbp)
    for step in range(nbp):
        dev.propagate(rng.normal(size=(nw, K)), 0.2)
    return dev, model.psi, (2, 2), h1e


def ueg_population(nw, nbp, seed=3):
    s = systems.UEG(2.0, 7, 3, 2.0)
    model = ueg_model_of(s)
    M, ne, K = s.nbasis, s.nup + s.ndown, 2 * len(s.qvecs)
    rng = numpy.random.RandomState(seed)
    dev = make_device(model, nw)
    dev.set(L.F_PHI, numpy.array([model.psi + 0.1 * (rng.rand(M, ne) + 1j * rng.rand(M, ne)) for _ in range(nw)]))
    dev.set(L.F_OT, dev.calc_overlap())
    dev.bp_configure(nbp)
    for step in range(nbp):
        dev.propagate(rng.normal(size=(nw, K)), 0.2)
    return dev, model.psi, (7, 3), None


def hubbard_population(nw, nbp):
    dev, BT2, psi, rng, U, dt = hirsch_device(4, 4, 3, 2, nw)
    dev.bp_configure(nbp)
    for step in range(nbp):
        dev.hirsch_kinetic()
        dev.hirsch_two_body(rng.random_sample((nw, dev.M)))
        dev.hirsch_finish(0.0)
    return dev, psi, (3, 2), None


def run_window(population, nw, restore=None, zero=(), energy=False, ekt=False, nbp=3):
    dev, psi, nelec, h1e = population(nw, nbp)
    try:
        w0 = dev.get(L.F_WEIGHT).copy()
        w0[list(zero)] = 0.0
        fock0 = None
        if ekt:                                   # the Fock matrices of a call without the new mode, on the same weights
            dev.set(L.F_WEIGHT, w0)
            dev.bp_observables(two_rdm=False, ekt=True, h1=h1e, L=None)
            fock0 = dev.bp_update(psi, 5, restore, energy, reset=False, ekt=True)[3]
        dev.bp_observables(two_rdm='correlation', ekt=ekt, h1=h1e, L=None)
        Gs, wts = [], []
        for i in range(nw):                       # every walker's G_bp and weight, as test_gpu_bp_obs.run_case does
            one = numpy.zeros(nw)
            one[i] = 1.0
            dev.set(L.F_WEIGHT, one)
            _, den, G = dev.bp_update(psi, 5, restore, reset=False)
            Gs.append(G / den)
            wts.append(den * w0[i])
        dev.set(L.F_WEIGHT, w0)
        E, den, G, extra = dev.bp_update(psi, 5, restore, energy, reset=False, two_rdm=True, ekt=ekt)
        two = extra['two_rdm']
        assert two.shape == (5, dev.M, dev.M)
        want = corr_ref.window(Gs, wts)
        err = numpy.max(numpy.abs(two - want)) / max(1.0, numpy.max(numpy.abs(want)))
        print("CORR-WINDOW | %s nw=%d restore=%s | rel err %.2e" % (population.__name__, nw, restore, err))
        close(den, numpy.sum(wts), 1e-10)
        close(two, want, TOL)
        # every G_bp[w] is idempotent with trace N: sum_j corr[2s+t][i,j] = N_t G_s[i,i], here on the weighted sums
        for s in range(2):
            for t in range(2):
                close(two[2 * s + t].sum(axis=1), nelec[t] * numpy.diag(G[s]), TOL)
        # the same window from the same state again: the same bits
        E2, den2, G2, extra2 = dev.bp_update(psi, 5, restore, energy, reset=False, two_rdm=True, ekt=ekt)
        assert numpy.array_equal(extra2['two_rdm'], two) and numpy.array_equal(E2, E)
        assert numpy.array_equal(G2, G) and den2 == den
        # without the option: afq_bp_update as before, bitwise the same sums
        a = dev.bp_update(psi, 5, restore, energy, reset=False)
        assert numpy.array_equal(a[2], G) and a[1] == den and numpy.array_equal(a[0], E)
        if not energy:
            assert not numpy.any(E)
        if ekt:
            assert numpy.array_equal(extra['fock_1p'], fock0['fock_1p'])
            assert numpy.array_equal(extra['fock_1h'], fock0['fock_1h'])
            dev.bp_observables(two_rdm='correlation')
            b = dev.bp_update(psi, 5, restore, energy, reset=False, two_rdm=True)
            assert numpy.array_equal(b[3]['two_rdm'], two)
    finally:
        dev.close()


@pytest.mark.parametrize("nw,energy", [(5, False), (5, True), (WCH + 3, True)])
def test_window_hubbard(nw, energy):
    """(3, 2) electrons on 4 x 4 sites, discrete fields; 35 walkers: two chunks of the walker sum and the pass over them."""
    run_window(hubbard_population, nw, energy=energy)


@pytest.mark.parametrize("restore,zero,ekt", [
    (None, (1, 3), False),
    ('partial', (1, 3), False),           # complex weights
    ('full', (1, 3), False),
    ('full', (1, 3), True),               # with the EKT: the Fock matrices of a call without the new mode
])
def test_window_generic(restore, zero, ekt):
    run_window(generic_population, 5, restore, zero, energy=ekt, ekt=ekt)


@pytest.mark.parametrize("energy", [False, True])
def test_window_ueg(energy):
    run_window(ueg_population, 4, energy=energy)


# ---------------------------------------------------------------- 3. through both driver loops
@pytest.mark.parametrize("batched", [False, True])
def test_traj_hubbard_correlations(golden, monkeypatch, tmp_path, batched):
    """The reference's discrete-field trajectory (the replay's own checks show the walk is unchanged); the energies are
    still hubbard_bp_energy.npz's, and U sum_i <n_i,up n_i,down> of the new array is every window's E2b."""
    got = capture_bp(monkeypatch)
    run_hirsch(golden, monkeypatch, 'traj_hirsch_bp.npz', basename=str(tmp_path / 'estimates'), batched=batched,
               bp={'tau_bp': 0.04, 'one_rdm': True, 'evaluate_energy': True, 'two_rdm': 'correlation'})
    est = got['est']
    want = golden('hubbard_bp_energy.npz')['bp_energies']
    U = float(golden('traj_hirsch_bp.npz')['U'])
    assert len(est.energies) == len(want) == len(est.two_rdm) == len(est.denominator)
    close(numpy.array(est.energies), want)
    for e, two, den in zip(est.energies, est.two_rdm, est.denominator):
        assert two.shape == (5, 16, 16) and two.dtype == numpy.complex128
        close(U * numpy.trace(two[1]) / den, e[2])
    den = numpy.array(est.denominator)
    two = extract_rdm(str(tmp_path / 'estimates.0.h5'), rdm_type='two_rdm')
    assert two.shape == (len(den), 5, 16, 16)
    assert numpy.array_equal(two, numpy.array(est.two_rdm) / den[:, None, None, None])


# ---------------------------------------------------------------- 4. refusals
def test_refusals():
    from tests.test_gpu_bp_msd import Case
    c = Case(12, 9, 3, 3, 2, 3)
    try:
        c.dev.bp_configure(3)
        with pytest.raises(L.AfqError) as e:
            c.dev.bp_observables(two_rdm='correlation')
        assert e.value.code == -5                           # AFQ_EUNSUPPORTED
    finally:
        c.dev.close()
    dev = make_device(build(12, 8, 2, 2)[0], 2)
    try:
        dev.bp_configure(2)
        rc = dev.lib.afq_bp_observables(dev.h, 4, 0, None, None, 0)
        assert rc == -1                                     # AFQ_EINVAL
        assert b'0, 1' in dev.lib.afq_last_error(dev.h) and b'3' in dev.lib.afq_last_error(dev.h)
        with pytest.raises(ValueError):
            dev.bp_observables(two_rdm='correlations')
        dev.bp_observables(two_rdm='correlation')           # and the handle stays usable
    finally:
        dev.close()
    dev = AfqDevice(0)                                      # no system yet
    try:
        G = numpy.zeros((1, 2, 4, 4), dtype=complex)
        out = numpy.zeros((1, 5, 4, 4), dtype=complex)
        assert dev.lib.afq_correlations_full_g(dev.h, _p(G), 1, _p(out)) == -2       # AFQ_ESTATE
        assert dev.lib.afq_correlations_full_g(dev.h, _p(G), 0, _p(out)) == -1
        assert dev.lib.afq_correlations_full_g(dev.h, None, 1, _p(out)) == -1
    finally:
        dev.close()
