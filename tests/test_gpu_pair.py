"""Back-propagated pairing correlations on the device (k_pair.hip): the kernel against the numpy restatement
(tests/pair_ref.py, itself checked against the Fock space in test_pair_cpu.py) on every tile and bond-block boundary it
has, the weighted sum around its chunk length with NaN-filled walkers of weight zero, the window's sums against
per-walker G_bp put through the restatement on all three systems, both driver loops on the reference's Hubbard
trajectory (where U sum_i pair[0, 0, i, i] must be the window's E2b), refusals, bitwise reproducibility, and the
neighbouring windows unchanged.

Tolerance: `close` of tests/test_gpu_traj.py at 1e-8 (error relative to max(1, max|want|)), the bound
test_gpu_corr.py, test_gpu_bp_obs.py and test_gpu_ueg_sf.py use for sums of this kind."""
import numpy
import pytest

from pauxy_amd import _lib as L
from pauxy_amd.device import AfqDevice, _p
from pauxy_amd.estimators.pairing import lattice_bonds
from pauxy_amd.utils.io import extract_rdm
from tests import pair_ref
from tests.helpers import make_device
from tests.test_gpu_bp_obs import build, capture_bp
from tests.test_gpu_corr import generic_population, hubbard_population, system_only_device, ueg_population
from tests.test_gpu_traj import close, run_hirsch
from tests.test_gpu_ueg_sf import rand_G

pytestmark = pytest.mark.gpu
TOL = 1e-8
T = 16              # tile edge of pair_tile_kernel (PT)
PB = 5              # bonds per block of pair_tile_kernel (PB)
WCH = 64            # Green's functions per chunk of the weighted sum (PAIR_WCH)
LATTICE = {15: (5, 3), 16: (4, 4), 33: (11, 3), 100: (10, 10), 130: (13, 10), 256: (16, 16)}


def relerr(got, want):
    return numpy.max(numpy.abs(got - want)) / max(1.0, numpy.max(numpy.abs(want)))


# ---------------------------------------------------------------- 1. the kernel
def table(M, nb):
    """The first nb bonds of the periodic lattice where M factors (and nb fits), else any table."""
    if M in LATTICE and nb <= 5:
        return lattice_bonds(*LATTICE[M])[0][:nb]
    return pair_ref.random_table(nb, M, 17 + M + nb)


_G = {}


def green(M, n):
    """Random complex G (not idempotent: nothing cancels), made once per shape."""
    if (M, n) not in _G:
        _G[(M, n)] = rand_G(n, M, 31 + M + n)
        _G[(M, n)].setflags(write=False)
    return _G[(M, n)]


def check_kernel(dev, G, nbr):
    dev.set_pairing_bonds(nbr)
    got = dev.pairing_full_g(G)
    again = dev.pairing_full_g(G)
    want = numpy.array([pair_ref.pair(g, nbr) for g in G])
    assert got.shape == want.shape == (len(G), len(nbr), len(nbr)) + G.shape[2:]
    print("PAIR-KERNEL | M=%d n=%d nb=%d | rel err %.2e" % (G.shape[-1], len(G), len(nbr), relerr(got, want)))
    close(got, want, TOL)
    assert numpy.array_equal(got, again)                    # same input, same bits
    return got


@pytest.mark.parametrize("nb", [1, 2, 5])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("M", [1, T - 1, T, T + 1, 2 * T + 1, 100, 130])
def test_kernel_on_every_tile_boundary(M, n, nb):
    G = green(M, n)
    dev = system_only_device('hubbard', M)
    try:
        check_kernel(dev, G, table(M, nb))
        check_kernel(dev, G, numpy.tile(numpy.arange(M, dtype=numpy.int32), (nb, 1)))       # the identity table
    finally:
        dev.close()


@pytest.mark.parametrize("kind", ['generic', 'ueg'])
def test_kernel_at_c4_size(kind):
    """16 x 16 sites, the five lattice bonds, on the other two kinds of handle (the kernel uses only M)."""
    G = green(256, 1)
    dev = system_only_device(kind, 256)
    try:
        check_kernel(dev, G, table(256, 5))
    finally:
        dev.close()


@pytest.mark.parametrize("M,nb", [(T + 1, PB + 1), (T + 1, 2 * PB), (2 * T + 1, 2 * PB + 1), (T - 1, 16)])
def test_kernel_on_every_bond_block_boundary(M, nb):
    """More than PB bonds: blocks of PB x PB bond pairs, the last ones partly empty."""
    dev = system_only_device('hubbard', M)
    try:
        nbr = table(M, nb)
        assert (nbr == -1).any()
        got = check_kernel(dev, green(M, 3), nbr)
        # a table that shrinks: nothing of the larger one is left
        small = check_kernel(dev, green(M, 3), nbr[1:3])
        assert numpy.array_equal(small, got[:, 1:3, 1:3])
    finally:
        dev.close()


def test_on_site_bond_is_the_double_occupancy_of_the_correlation_functions():
    M = 2 * T + 1
    G = green(M, 3)
    dev = system_only_device('hubbard', M)
    try:
        dev.set_pairing_bonds(lattice_bonds(11, 3)[0])
        pair = dev.pairing_full_g(G)
        corr = dev.correlations_full_g(G)
    finally:
        dev.close()
    d = numpy.arange(M)
    close(pair[:, 0, 0, d, d], corr[:, 1, d, d], TOL)            # <n_i,up n_i,down> = G_0[i,i] G_1[i,i]


# ---------------------------------------------------------------- 2. the window
def poisoned_population(nw, nbp, dead, seed=5):
    """generic_population of test_gpu_corr.py with walkers whose phi_old is NaN: the walk itself is sane (phi is put back
    before the first step), every G_bp of a walker in `dead` is NaN."""
    model, h1e, Lv, rng = build(12, 8, 2, 2, seed)
    M, ne, K = 12, 4, 8
    dev = make_device(model, nw)
    phi = numpy.array([model.psi + 0.1 * (rng.rand(M, ne) + 1j * rng.rand(M, ne)) for _ in range(nw)])
    bad = phi.copy()
    bad[list(dead)] = numpy.nan
    dev.set(L.F_PHI, bad)
    dev.bp_configure(nbp)                         # phi_old = phi
    dev.set(L.F_PHI, phi)
    dev.set(L.F_OT, dev.calc_overlap())
    for step in range(nbp):
        dev.propagate(rng.normal(size=(nw, K)), 0.2)
    return dev, model.psi, (2, 2), h1e


def per_walker(dev, psi, nw, w0, restore):
    """Every walker's G_bp and accumulation weight, as test_gpu_bp_obs.run_case takes them."""
    Gs, wts = [], []
    for i in range(nw):
        one = numpy.zeros(nw)
        one[i] = 1.0
        dev.set(L.F_WEIGHT, one)
        _, den, G = dev.bp_update(psi, 5, restore, reset=False)
        Gs.append(G / den)
        wts.append(den * w0[i])
    dev.set(L.F_WEIGHT, w0)
    return Gs, wts


@pytest.mark.parametrize("nw", [WCH - 1, WCH, WCH + 1, 2 * WCH + 1])
def test_weighted_sum_around_the_chunk_length(nw):
    """One chunk, a full one, two and three (the pass over the partial sums), with NaN-filled Green's functions of
    weight zero at the ends of the chunks and inside them: they are left out whatever they hold."""
    dead = sorted(set([0, 7, WCH - 1, WCH, nw - 1]) & set(range(nw)))
    dev, psi, nelec, h1e = poisoned_population(nw, 2, dead)
    try:
        nbr = pair_ref.random_table(3, dev.M, 4)
        dev.set_pairing_bonds(nbr)
        dev.bp_observables(two_rdm='pairing')
        w0 = dev.get(L.F_WEIGHT).copy()
        assert numpy.all(numpy.isfinite(w0)) and numpy.all(w0 != 0)
        w0[dead] = 0.0
        # the accumulation weights one walker at a time (the denominator is a sum of weights alone: no NaN reaches it)
        wts = []
        for i in range(nw):
            one = numpy.zeros(nw)
            one[i] = 1.0
            dev.set(L.F_WEIGHT, one)
            wts.append(dev.bp_update(psi, 5, 'partial', reset=False)[1] * w0[i])
        dev.set(L.F_WEIGHT, w0)
        assert numpy.all(numpy.isfinite(wts)) and all(wts[i] == 0 for i in dead)
        two = dev.bp_update(psi, 5, 'partial', reset=False, two_rdm=True)[3]['two_rdm']
        Gs = dev.get(L.F_G).copy()                  # the window's G_bp of every walker, as the kernel read them
        assert all(numpy.any(numpy.isnan(Gs[i])) for i in dead)
        assert all(numpy.all(numpy.isfinite(Gs[i])) for i in range(nw) if i not in dead)
        want = pair_ref.window(Gs, wts, nbr)
        assert two.shape == (3, 3, dev.M, dev.M)
        print("PAIR-WSUM | nw=%d | rel err %.2e" % (nw, relerr(two, want)))
        close(two, want, TOL)
        again = dev.bp_update(psi, 5, 'partial', reset=False, two_rdm=True)[3]['two_rdm']
        assert numpy.array_equal(two, again)
    finally:
        dev.close()


def run_window(population, nbr_of, nw, restore=None, zero=(), energy=False, ekt=False, nbp=3):
    dev, psi, nelec, h1e = population(nw, nbp)
    try:
        nbr = nbr_of(dev.M)
        nb = len(nbr)
        w0 = dev.get(L.F_WEIGHT).copy()
        w0[list(zero)] = 0.0
        dev.set(L.F_WEIGHT, w0)
        # a call without the mode, on the same weights: its estimates and Fock matrices
        if ekt:
            dev.bp_observables(two_rdm=False, ekt=True, h1=h1e, L=None)
        base = dev.bp_update(psi, 5, restore, energy, reset=False, ekt=ekt)
        dev.set_pairing_bonds(nbr)
        dev.bp_observables(two_rdm='pairing', ekt=ekt, h1=h1e, L=None)
        Gs, wts = per_walker(dev, psi, nw, w0, restore)
        E, den, G, extra = dev.bp_update(psi, 5, restore, energy, reset=False, two_rdm=True, ekt=ekt)
        two = extra['two_rdm']
        assert two.shape == (nb, nb, dev.M, dev.M)
        want = pair_ref.window(Gs, wts, nbr)
        print("PAIR-WINDOW | %s nw=%d restore=%s energy=%s ekt=%s | rel err %.2e" % (
            population.__name__, nw, restore, energy, ekt, relerr(two, want)))
        close(den, numpy.sum(wts), 1e-10)
        close(two, want, TOL)
        assert numpy.max(numpy.abs(want)) > 1e-3
        # est_out and the Fock matrices are those of the call without the mode, bit for bit
        assert numpy.array_equal(E, base[0]) and den == base[1] and numpy.array_equal(G, base[2])
        if not energy:
            assert not numpy.any(E)
        if ekt:
            assert numpy.array_equal(extra['fock_1p'], base[3]['fock_1p'])
            assert numpy.array_equal(extra['fock_1h'], base[3]['fock_1h'])
        # the same window from the same state again: the same bits; and afq_bp_update as before
        E2, den2, G2, extra2 = dev.bp_update(psi, 5, restore, energy, reset=False, two_rdm=True, ekt=ekt)
        assert numpy.array_equal(extra2['two_rdm'], two) and numpy.array_equal(E2, E)
        a = dev.bp_update(psi, 5, restore, energy, reset=False)
        assert numpy.array_equal(a[2], G) and a[1] == den and numpy.array_equal(a[0], E)
        if ekt:
            # the mode without the EKT, and the EKT after the mode was taken out again
            dev.bp_observables(two_rdm='pairing')
            b = dev.bp_update(psi, 5, restore, energy, reset=False, two_rdm=True)
            assert numpy.array_equal(b[3]['two_rdm'], two)
            dev.bp_observables(two_rdm=False, ekt=True, h1=h1e, L=None)
            c = dev.bp_update(psi, 5, restore, energy, reset=False, ekt=True)
            assert numpy.array_equal(c[3]['fock_1p'], base[3]['fock_1p'])
    finally:
        dev.close()


@pytest.mark.parametrize("nw,energy", [(5, False), (5, True), (WCH + 3, True)])
def test_window_hubbard(nw, energy):
    """(3, 2) electrons on 4 x 4 sites, discrete fields, the five lattice bonds; 67 walkers: two chunks."""
    run_window(hubbard_population, lambda M: lattice_bonds(4, 4)[0], nw, energy=energy)


@pytest.mark.parametrize("restore,zero,energy,ekt", [
    (None, (1, 3), False, False),
    ('partial', (1, 3), True, False),     # complex weights
    ('full', (1, 3), False, False),
    ('full', (1, 3), True, True),         # with the EKT: the Fock matrices of a call without the mode
    ('partial', (), False, True),         # the EKT without the energies
])
def test_window_generic(restore, zero, energy, ekt):
    run_window(generic_population, lambda M: pair_ref.random_table(3, M, 6), 5, restore, zero, energy=energy, ekt=ekt)


@pytest.mark.parametrize("energy", [False, True])
def test_window_ueg(energy):
    run_window(ueg_population, lambda M: pair_ref.random_table(2, M, 8), 4, energy=energy)


# ---------------------------------------------------------------- 3. through both driver loops
@pytest.mark.parametrize("batched", [False, True])
def test_traj_hubbard_pairing(golden, monkeypatch, tmp_path, batched):
    """The reference's discrete-field trajectory (the replay's own checks show the walk is unchanged); the energies are
    still hubbard_bp_energy.npz's, and U sum_i <n_i,up n_i,down> from the on-site bond is every window's E2b."""
    got = capture_bp(monkeypatch)
    run_hirsch(golden, monkeypatch, 'traj_hirsch_bp.npz', basename=str(tmp_path / 'estimates'), batched=batched,
               bp={'tau_bp': 0.04, 'one_rdm': True, 'evaluate_energy': True, 'two_rdm': 'pairing'})
    est = got['est']
    want = golden('hubbard_bp_energy.npz')['bp_energies']
    U = float(golden('traj_hirsch_bp.npz')['U'])
    assert len(est.energies) == len(want) == len(est.two_rdm) == len(est.denominator)
    close(numpy.array(est.energies), want)
    nbr = lattice_bonds(4, 4)[0]
    for e, two, den, one in zip(est.energies, est.two_rdm, est.denominator, est.one_rdm):
        assert two.shape == (5, 5, 16, 16) and two.dtype == numpy.complex128
        close(U * numpy.trace(two[0, 0]) / den, e[2])
        # <D+(i, i_b) D(i, i_b)> = <n_i,up n_ib,down> on the diagonal of every bond: summed over i and the four
        # neighbour bonds it is real and positive
        assert all(numpy.trace(two[b, b]).real / den.real > 0 for b in range(5))
    den = numpy.array(est.denominator)
    two = extract_rdm(str(tmp_path / 'estimates.0.h5'), rdm_type='two_rdm')
    assert two.shape == (len(den), 5, 5, 16, 16)
    assert numpy.array_equal(two, numpy.array(est.two_rdm) / den[:, None, None, None, None])
    assert nbr.shape == (5, 16)


# ---------------------------------------------------------------- 4. refusals
def test_refusals():
    from tests.test_gpu_bp_msd import Case
    c = Case(12, 9, 3, 3, 2, 3)
    try:
        c.dev.bp_configure(3)
        c.dev.set_pairing_bonds(pair_ref.chain_table(12))
        with pytest.raises(L.AfqError) as e:
            c.dev.bp_observables(two_rdm='pairing')
        assert e.value.code == L.AFQ_EUNSUPPORTED
        assert c.dev.lib.afq_bp_pairing(c.dev.h, 1) == L.AFQ_EUNSUPPORTED
        assert c.dev.pairing_full_g(rand_G(1, 12, 1)).shape == (1, 3, 3, 12, 12)       # the kernel itself is not refused
    finally:
        c.dev.close()
    dev = make_device(build(12, 8, 2, 2)[0], 2)
    lib, M = dev.lib, dev.M
    try:
        chain = pair_ref.chain_table(M)
        assert lib.afq_bp_pairing(dev.h, 1) == L.AFQ_ESTATE                     # before afq_bp_configure
        assert b'afq_bp_configure' in lib.afq_last_error(dev.h)
        dev.bp_configure(2)
        assert lib.afq_bp_pairing(dev.h, 1) == L.AFQ_ESTATE                     # no bond table
        assert b'afq_set_pairing_bonds' in lib.afq_last_error(dev.h)
        G = rand_G(1, M, 2)
        out = numpy.zeros((1, 3, 3, M, M), dtype=complex)
        assert lib.afq_pairing_full_g(dev.h, _p(G), 1, _p(out)) == L.AFQ_ESTATE
        with pytest.raises(L.AfqError) as e:
            dev.bp_observables(two_rdm='pairing')
        assert e.value.code == L.AFQ_ESTATE
        dev.set_pairing_bonds(chain)
        for bad, where in ((M, b'nbr[1][3]'), (-2, b'nbr[1][3]')):              # a table entry out of range
            t = chain.copy()
            t[1, 3] = bad
            assert lib.afq_set_pairing_bonds(dev.h, 3, _p(t)) == L.AFQ_EINVAL
            assert where in lib.afq_last_error(dev.h) and str(bad).encode() in lib.afq_last_error(dev.h)
        many = numpy.tile(chain[:1], (17, 1))
        assert lib.afq_set_pairing_bonds(dev.h, 17, _p(many)) == L.AFQ_EINVAL   # nb > 16, by number
        assert b'17' in lib.afq_last_error(dev.h)
        assert lib.afq_set_pairing_bonds(dev.h, -1, _p(many)) == L.AFQ_EINVAL
        assert lib.afq_set_pairing_bonds(dev.h, 3, None) == L.AFQ_EINVAL
        with pytest.raises(ValueError):
            dev.set_pairing_bonds(chain[:, :M - 1])
        # the refused tables left the one before in place, and the handle usable
        close(dev.pairing_full_g(G)[0], pair_ref.pair(G[0], chain), TOL)
        dev.set_pairing_bonds(many[:16])                                        # 16 bonds are taken
        close(dev.pairing_full_g(G)[0], pair_ref.pair(G[0], many[:16]), TOL)
        dev.set_pairing_bonds(chain)
        assert lib.afq_pairing_full_g(dev.h, _p(G), 0, _p(out)) == L.AFQ_EINVAL
        assert lib.afq_pairing_full_g(dev.h, None, 1, _p(out)) == L.AFQ_EINVAL
        # afq_bp_observables answers as before
        rc = lib.afq_bp_observables(dev.h, 4, 0, None, None, 0)
        assert rc == L.AFQ_EINVAL
        assert b'0, 1' in lib.afq_last_error(dev.h) and b'3' in lib.afq_last_error(dev.h)
        with pytest.raises(ValueError):
            dev.bp_observables(two_rdm='correlations')
        with pytest.raises(ValueError) as e:
            dev.bp_observables(two_rdm='pairings')
        assert 'pairing' in str(e.value)
        dev.bp_observables(two_rdm='pairing')
        psi = build(12, 8, 2, 2)[0].psi
        assert dev.bp_update(psi, 5, None, reset=False, two_rdm=True)[3]['two_rdm'].shape == (3, 3, M, M)
        # a new table ends the mode (the slot was sized for the old one); nb = 0 clears the table
        dev.set_pairing_bonds(chain[:2])
        two = numpy.zeros((2, 2, M, M), dtype=complex)
        est = numpy.zeros(4 + 2 * M * M, dtype=complex)
        phi0 = numpy.ascontiguousarray(psi, dtype=complex)
        assert lib.afq_bp_update_ext(dev.h, _p(phi0), 5, 0, 0, 0, _p(est), _p(two), None) == L.AFQ_ESTATE
        dev.bp_observables(two_rdm='pairing')
        assert dev.bp_update(psi, 5, None, reset=False, two_rdm=True)[3]['two_rdm'].shape == (2, 2, M, M)
        assert lib.afq_bp_pairing(dev.h, 0) == 0
        assert lib.afq_bp_update_ext(dev.h, _p(phi0), 5, 0, 0, 0, _p(est), _p(two), None) == L.AFQ_ESTATE
        dev.set_pairing_bonds(None)
        assert lib.afq_bp_pairing(dev.h, 1) == L.AFQ_ESTATE
        dev.bp_observables(two_rdm='correlation')                               # and the handle stays usable
        assert dev.bp_update(psi, 5, None, reset=False, two_rdm=True)[3]['two_rdm'].shape == (5, M, M)
    finally:
        dev.close()
    dev = AfqDevice(0)                                      # no system yet
    try:
        t = numpy.zeros((1, 4), dtype=numpy.int32)
        assert dev.lib.afq_set_pairing_bonds(dev.h, 1, _p(t)) == L.AFQ_ESTATE
        G = numpy.zeros((1, 2, 4, 4), dtype=complex)
        out = numpy.zeros((1, 1, 1, 4, 4), dtype=complex)
        assert dev.lib.afq_pairing_full_g(dev.h, _p(G), 1, _p(out)) == L.AFQ_ESTATE
    finally:
        dev.close()


# ---------------------------------------------------------------- 5. the neighbours
def neighbour_window(population, mode):
    dev, psi, nelec, h1e = population(5, 3)
    try:
        dev.bp_observables(two_rdm=mode)
        return dev.bp_update(psi, 5, None, True, reset=False, two_rdm=True)
    finally:
        dev.close()


def test_neighbouring_windows_are_unchanged():
    """A correlation window and a structure-factor window before and after a handle in pairing mode lived, and on a
    handle that was in pairing mode in between: the same bits."""
    before = [neighbour_window(hubbard_population, 'correlation'), neighbour_window(ueg_population, 'structure_factor')]
    dev, psi, nelec, h1e = ueg_population(5, 3)
    try:
        dev.set_pairing_bonds(pair_ref.random_table(6, dev.M, 9))
        dev.bp_observables(two_rdm='pairing')
        assert dev.bp_update(psi, 5, None, True, reset=False, two_rdm=True)[3]['two_rdm'].shape == (6, 6, dev.M, dev.M)
        dev.bp_observables(two_rdm='structure_factor')
        same = dev.bp_update(psi, 5, None, True, reset=False, two_rdm=True)
    finally:
        dev.close()
    after = [neighbour_window(hubbard_population, 'correlation'), neighbour_window(ueg_population, 'structure_factor')]
    for a, b in zip(before + [before[1]], after + [same]):
        assert numpy.array_equal(a[0], b[0]) and a[1] == b[1] and numpy.array_equal(a[2], b[2])
        assert numpy.array_equal(a[3]['two_rdm'], b[3]['two_rdm'])
        assert numpy.any(a[3]['two_rdm'])
