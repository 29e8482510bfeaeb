"""Back-propagated pairing correlations, the parts that need no GPU: the numpy restatement (tests/pair_ref.py) against
brute-force enumeration of the Fock space, the bond tables and identities of estimators/pairing.py, and the
BackPropagation façade with ``two_rdm: 'pairing'``."""
import types

import numpy
import pytest

from pauxy_amd import systems
from pauxy_amd.estimators import pairing
from pauxy_amd.estimators.back_propagation import BackPropagation
from tests import corr_ref, pair_ref
from tests.test_corr_cpu import Fock
from tests.test_ueg_sf_cpu import QMC, Comm, generic, make_bp


def determinants(M, na, nb, seed):
    rng = numpy.random.RandomState(seed)
    cr = lambda *s: rng.normal(size=s) + 1j * rng.normal(size=s)
    return [cr(M, na), cr(M, nb)], [cr(M, na), cr(M, nb)]         # random, complex, not orthogonal


def greens(L, R):
    """G_s[i, j] = <c+_is c_js> = [R_s (L_s^H R_s)^-1 L_s^H]^T"""
    return numpy.array([(R[s] @ numpy.linalg.inv(L[s].conj().T @ R[s]) @ L[s].conj().T).T for s in range(2)])


# ---------------------------------------------------------------- 1. the restatement against the Fock space
@pytest.mark.parametrize("table", ['chain', 'random'])
@pytest.mark.parametrize("na,nb", [(2, 1), (2, 2)])
def test_restatement_against_fock_space_enumeration(na, nb, table):
    M = 4
    L, R = determinants(M, na, nb, 7 + na + nb)
    nbr = pair_ref.chain_table(M) if table == 'chain' else pair_ref.random_table(3, M, 2)
    if table == 'random':
        assert (nbr == -1).any() and any(len(set(row[row >= 0])) < (row >= 0).sum() for row in nbr)
    f = Fock(2 * M)                                               # spin-orbital of (site i, spin s): s * M + i

    def embed(D):
        orbs = numpy.zeros((2 * M, na + nb), dtype=complex)
        orbs[:M, :na], orbs[M:, na:] = D[0], D[1]
        return orbs
    bra, ket = f.determinant(embed(L)), f.determinant(embed(R))
    ovlp = numpy.vdot(bra, ket)
    ev = lambda v: numpy.vdot(bra, v) / ovlp
    G = greens(L, R)
    n = len(nbr)
    want = numpy.zeros((n, n, M, M), dtype=complex)
    for b in range(n):
        for c in range(n):
            for i in range(M):
                for j in range(M):
                    ib, jc = nbr[b][i], nbr[c][j]
                    if ib < 0 or jc < 0:
                        continue
                    # D+(i, ib) D(j, jc) = c+_i,up c+_ib,down c_jc,down c_j,up
                    want[b, c, i, j] = ev(f.cre(i, f.cre(M + ib, f.ann(M + jc, f.ann(j, ket)))))
    got = pair_ref.pair(G, nbr)
    assert numpy.max(numpy.abs(want)) > 1e-3
    assert numpy.max(numpy.abs(got - want)) < 1e-12
    # the transposed convention gives the array with both index pairs exchanged
    gt = pair_ref.pair(G.transpose(0, 2, 1), nbr)
    assert numpy.max(numpy.abs(gt - want.transpose(1, 0, 3, 2))) < 1e-12
    # a -1 gives 0 whatever G holds, and the sum over walkers in extended precision is the plain sum here
    Gn = G.copy()
    Gn[1, 0, :] = numpy.nan
    assert not numpy.isnan(pair_ref.pair(Gn, numpy.full((1, M), -1))).any()
    w = [0.3 + 0.1j, 2.0, 0.0]
    ws = pair_ref.window([G, 2 * G, Gn], w, nbr)
    assert numpy.max(numpy.abs(ws - (w[0] * got + w[1] * pair_ref.pair(2 * G, nbr)))) < 1e-12


# ---------------------------------------------------------------- 2. lattice_bonds
@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("nx,ny", [(4, 4), (3, 2), (5, 1)])
def test_lattice_bonds(nx, ny, periodic):
    nbr, inverse = pairing.lattice_bonds(nx, ny, periodic)
    M = nx * ny
    nb = 5 if ny > 1 else 3
    assert nbr.shape == (nb, M) and nbr.dtype == numpy.int32 and len(inverse) == nb
    assert numpy.array_equal(nbr[0], numpy.arange(M))
    assert nbr.min() >= -1 and nbr.max() < M
    assert periodic == (not (nbr == -1).any())
    for b in range(nb):
        for i in range(M):
            if nbr[b][i] >= 0:
                assert nbr[inverse[b]][nbr[b][i]] == i
    # the displacements, in the order on-site, +x, -x, +y, -y, with i = ix + nx iy
    steps = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)][:nb]
    for b, (dx, dy) in enumerate(steps):
        for i in range(M):
            jx, jy = i % nx + dx, i // nx + dy
            inside = 0 <= jx < nx and 0 <= jy < ny
            want = (jx % nx) + nx * (jy % ny) if (periodic or inside) else -1
            assert nbr[b][i] == want
    if periodic and ny > 1:
        # the neighbours of the hopping matrix of systems.Hubbard (where no two bonds coincide)
        T = systems.Hubbard(4, 4, 1, 1, 4.0).T[0]
        n4 = pairing.lattice_bonds(4, 4)[0]
        for i in range(16):
            assert sorted(n4[1:, i]) == sorted(numpy.nonzero(T[i])[0])


# ---------------------------------------------------------------- 3. singlet, channels, uncorrelated
def test_singlet_is_hermitian_and_counts_double_occupancy():
    nx, ny = 3, 2
    M, na, nb = nx * ny, 3, 2
    L, _ = determinants(M, na, nb, 4)
    G = greens(L, L)                                              # bra = ket
    for periodic in (True, False):
        nbr, inverse = pairing.lattice_bonds(nx, ny, periodic)
        ps = pairing.singlet(pair_ref.pair(G, nbr), nbr, inverse)
        assert ps.shape == (5, 5, M, M)
        assert numpy.max(numpy.abs(ps - ps.transpose(1, 0, 3, 2).conj())) < 1e-12
        docc = numpy.diag(corr_ref.corr(G)[1])                    # <n_i,up n_i,down>
        assert numpy.max(numpy.abs(numpy.diag(ps[0, 0]) - 2 * docc)) < 1e-12
        assert numpy.max(numpy.abs(ps[0, 0] - 2 * G[0] * G[1])) < 1e-12
        # written out for one element: 1/2 of the four terms
        b, c, i, j = 1, 3, 0, 1
        ib, jc = nbr[b][i], nbr[c][j]
        if ib >= 0 and jc >= 0:
            want = 0.5 * (G[0][i, j] * G[1][ib, jc] + G[0][i, jc] * G[1][ib, j]
                          + G[0][ib, j] * G[1][i, jc] + G[0][ib, jc] * G[1][i, j])
            assert abs(ps[b, c, i, j] - want) < 1e-12
        # where a partner is missing there is no pair field
        gone = nbr < 0
        assert not numpy.any(ps[gone[:, None, :, None] | gone[None, :, None, :]])
        # the transposed convention in, the transposed form of the result out
        pt = pairing.singlet(pair_ref.pair(G.transpose(0, 2, 1), nbr), nbr, inverse)
        assert numpy.max(numpy.abs(pt.transpose(1, 0, 3, 2) - ps)) < 1e-12


def test_channels_of_a_hand_built_array():
    M = 2
    c = numpy.array([[1.0, 2.0], [3.0, 4.0]])
    ps = numpy.zeros((5, 5, M, M))
    ps[1, 1], ps[1, 3], ps[4, 2], ps[0, 0], ps[0, 4] = c, 10 * c, 100 * c, 1000 * c, 7 * c
    assert numpy.array_equal(pairing.channel(ps, pairing.s_wave()), 1000 * c)
    # d-wave: (+x, +x) 1/4, (+x, +y) -1/4, (-y, -x) -1/4
    assert numpy.allclose(pairing.channel(ps, pairing.d_wave()), (0.25 - 2.5 - 25.0) * c, rtol=0, atol=1e-13)
    assert numpy.allclose(pairing.channel(ps, pairing.extended_s()), (0.25 + 2.5 + 25.0) * c, rtol=0, atol=1e-13)
    assert numpy.array_equal(pairing.d_wave(), [0, 0.5, 0.5, -0.5, -0.5])
    assert numpy.array_equal(pairing.extended_s(), [0, 0.5, 0.5, 0.5, 0.5])
    assert numpy.allclose(pairing.extended_s(3), [0, 0.5 ** 0.5, 0.5 ** 0.5]) and numpy.array_equal(pairing.s_wave(3), [1, 0, 0])
    with pytest.raises(ValueError):
        pairing.d_wave(3)


def test_uncorrelated_is_the_pairing_array_of_one_determinant_pair():
    M = 6
    L, R = determinants(M, 3, 2, 9)
    G = greens(L, R)
    for nbr in (pairing.lattice_bonds(3, 2, False)[0], pair_ref.random_table(4, M, 3)):
        assert numpy.array_equal(pairing.uncorrelated(G, nbr), pair_ref.pair(G, nbr))


# ---------------------------------------------------------------- 4. the façade
def test_back_propagation_accepts_pairing():
    s = systems.Hubbard(4, 4, 7, 7, 4.0)
    M = s.nbasis
    est = make_bp({'two_rdm': 'pairing'}, s)
    assert est.pairing and not est.correlation and not est.structure_factor and est.two_rdm == []
    assert not BackPropagation.pairing
    assert numpy.array_equal(est.pairing_bonds, pairing.lattice_bonds(4, 4)[0])
    assert est.two_rdm_shape == (5, 5, M, M)
    assert est.estimates.size == 3 + 1 + 2 * M * M + 25 * M * M
    assert make_bp({'two_rdm': 'pairing', 'evaluate_energy': True}, s).estimates.size == est.estimates.size
    chain = pair_ref.chain_table(M)
    assert make_bp({'two_rdm': 'pairing', 'pairing_bonds': chain}, s).two_rdm_shape == (3, 3, M, M)
    assert not make_bp({'two_rdm': 'correlation'}, s).pairing


@pytest.mark.parametrize("one_rdm", [True, False])
def test_back_propagation_slicing_with_ekt(one_rdm):
    """The [nb, nb, M, M] block sits where the other two_rdm forms sit; the Fock matrices follow it."""
    s = generic()
    M = s.nbasis
    nbr = pair_ref.random_table(2, M, 1)
    est = make_bp({'two_rdm': 'pairing', 'pairing_bonds': nbr, 'evaluate_ekt': True, 'one_rdm': one_rdm}, s)
    assert est.estimates.size == 3 + 1 + 2 * M * M + 4 * M * M + 2 * M * M
    est.estimates[:] = numpy.arange(est.estimates.size) + 0.5j
    est.accumulated = True
    est.buff_ix = 5
    flat = est.estimates.copy()
    est.print_step(Comm(), 1, 0)
    start = 4 + 2 * M * M
    assert est.two_rdm[0].shape == (2, 2, M, M) and est.two_rdm[0].dtype == numpy.complex128
    assert numpy.array_equal(est.two_rdm[0].ravel(), flat[start:start + 4 * M * M])
    fock = 4 + (2 * M * M if one_rdm else 0) + 4 * M * M          # the reference's slicing (back_propagation.py:310-324)
    assert numpy.array_equal(est.fock_1p[0].ravel(), flat[fock:fock + M * M])
    assert numpy.array_equal(est.fock_1h[0].ravel(), flat[fock + M * M:fock + 2 * M * M])


def test_back_propagation_refusals():
    s = generic()
    M = s.nbasis
    nbr = pair_ref.chain_table(M)
    with pytest.raises(NotImplementedError):
        BackPropagation({'tau_bp': 0.025, 'two_rdm': 'pairing', 'pairing_bonds': nbr}, True, None, QMC, s,
                        types.SimpleNamespace(ndets=3), complex, None)
    with pytest.raises(ValueError):                               # no lattice to take the bonds from
        make_bp({'two_rdm': 'pairing'}, s)
    for bad in (nbr[:, :M - 1], nbr.astype(float), numpy.where(nbr == 0, M, nbr), numpy.where(nbr == 0, -2, nbr),
                numpy.repeat(nbr, 6, axis=0), nbr[0]):
        with pytest.raises(ValueError):
            make_bp({'two_rdm': 'pairing', 'pairing_bonds': bad}, s)
    # the existing refusals stay
    with pytest.raises(ValueError):
        make_bp({'two_rdm': 'correlations'}, s)
    with pytest.raises(ValueError) as e:
        make_bp({'two_rdm': 'pairings'}, s)
    assert 'pairing' in str(e.value) and 'correlation' in str(e.value)
    with pytest.raises(NotImplementedError):
        make_bp({'two_rdm': 'structure_factor'}, s)
