"""Back-propagated density and spin correlation functions, the parts that need no GPU: the numpy restatement
(tests/corr_ref.py) against brute-force enumeration of the Fock space, the identities of estimators/correlation.py, and
the BackPropagation façade with ``two_rdm: 'correlation'``."""
import types

import numpy
import pytest

from pauxy_amd import systems
from pauxy_amd.estimators.back_propagation import BackPropagation
from pauxy_amd.estimators.correlation import spin_charge, translation_average
from tests import corr_ref
from tests.test_ueg_sf_cpu import QMC, Comm, generic, make_bp, ueg


# ---------------------------------------------------------------- 1. the restatement against the Fock space
class Fock(object):
    """Fermions on nso spin-orbitals, states as vectors over the 2^nso occupation-number bit strings; orbital p is bit p
    and the sign of c_p / c+_p is the parity of the occupied orbitals below p."""

    def __init__(self, nso):
        self.nso, self.dim = nso, 1 << nso
        self.idx = numpy.arange(self.dim)
        pop = numpy.array([bin(i).count('1') for i in range(self.dim)])
        self.sign = [1.0 - 2.0 * (pop[self.idx & ((1 << p) - 1)] & 1) for p in range(nso)]

    def ann(self, p, v):
        occ = ((self.idx >> p) & 1) == 1
        out = numpy.zeros_like(v)
        out[self.idx[occ] ^ (1 << p)] = self.sign[p][occ] * v[occ]
        return out

    def cre(self, p, v):
        emp = ((self.idx >> p) & 1) == 0
        out = numpy.zeros_like(v)
        out[self.idx[emp] | (1 << p)] = self.sign[p][emp] * v[emp]
        return out

    def num(self, p, v):
        return self.cre(p, self.ann(p, v))

    def determinant(self, orbs):
        """prod_k (sum_p orbs[p, k] c+_p) |0>"""
        v = numpy.zeros(self.dim, dtype=complex)
        v[0] = 1.0
        for k in reversed(range(orbs.shape[1])):
            v = sum(orbs[p, k] * self.cre(p, v) for p in range(self.nso))
        return v


def test_restatement_against_fock_space_enumeration():
    M, na, nb = 5, 2, 1
    rng = numpy.random.RandomState(5)
    cr = lambda *s: rng.normal(size=s) + 1j * rng.normal(size=s)
    L, R = [cr(M, na), cr(M, nb)], [cr(M, na), cr(M, nb)]         # random, complex, not orthogonal
    f = Fock(2 * M)                                               # spin-orbital of (site i, spin s): s * M + i

    def embed(D):
        orbs = numpy.zeros((2 * M, na + nb), dtype=complex)
        orbs[:M, :na], orbs[M:, na:] = D[0], D[1]
        return orbs
    bra, ket = f.determinant(embed(L)), f.determinant(embed(R))
    ovlp = numpy.vdot(bra, ket)
    ev = lambda v: numpy.vdot(bra, v) / ovlp
    # G_s[i, j] = <c+_is c_js> = [R_s (L_s^H R_s)^-1 L_s^H]^T, checked on the way
    G = numpy.array([(R[s] @ numpy.linalg.inv(L[s].conj().T @ R[s]) @ L[s].conj().T).T for s in range(2)])
    for s in range(2):
        for i in range(M):
            for j in range(M):
                assert abs(ev(f.cre(s * M + i, f.ann(s * M + j, ket))) - G[s, i, j]) < 1e-12
    want = numpy.zeros((5, M, M), dtype=complex)
    for i in range(M):
        for j in range(M):
            for s in range(2):
                for t in range(2):
                    want[2 * s + t, i, j] = ev(f.num(s * M + i, f.num(t * M + j, ket)))
            # S+_i S-_j = c+_i,up c_i,down c+_j,down c_j,up
            want[4, i, j] = ev(f.cre(i, f.ann(M + i, f.cre(M + j, f.ann(j, ket)))))
    got = corr_ref.corr(G)
    assert numpy.max(numpy.abs(got - want)) < 1e-12
    # slices 0-3 do not change with the convention of G, slice 4 is transposed with it
    gt = corr_ref.corr(G.transpose(0, 2, 1))
    assert numpy.max(numpy.abs(gt[:4] - want[:4])) < 1e-12
    assert numpy.max(numpy.abs(gt[4] - want[4].T)) < 1e-12
    # the sum over walkers in extended precision is the plain sum here
    w = [0.3 + 0.1j, 2.0]
    assert numpy.max(numpy.abs(corr_ref.window([G, 2 * G], w) - (w[0] * got + w[1] * corr_ref.corr(2 * G)))) < 1e-12


# ---------------------------------------------------------------- 2. spin_charge
def test_spin_charge_identities():
    """A high-spin determinant with L = R (the down orbitals span a subspace of the up ones) is an eigenstate of S^2
    with S = (na - nb) / 2: sum_ij <S_i . S_j> = S (S + 1); and sum_j <n_i n_j> = N n_i on any state of N particles."""
    M, na, nb = 7, 4, 2
    rng = numpy.random.RandomState(8)
    A = numpy.linalg.qr(rng.normal(size=(M, na)) + 1j * rng.normal(size=(M, na)))[0]
    U = numpy.linalg.qr(rng.normal(size=(na, na)) + 1j * rng.normal(size=(na, na)))[0]
    B = (A @ U)[:, :nb]
    for transpose in (False, True):
        G = numpy.array([(A @ A.conj().T).T, (B @ B.conj().T).T])          # idempotent, traces na and nb
        if transpose:
            G = G.transpose(0, 2, 1).copy()
        charge, szsz, ss = spin_charge(corr_ref.corr(G), G)
        S = 0.5 * (na - nb)
        assert abs(ss.sum() - S * (S + 1)) < 1e-12
        assert abs(szsz.sum() - S * S) < 1e-12
        n = numpy.diag(G[0]) + numpy.diag(G[1])
        assert numpy.max(numpy.abs(charge.sum(axis=1) - (na + nb) * n)) < 1e-12
        c = corr_ref.corr(G)                        # the sum rule of every slice: sum_j corr[2s+t][i,j] = N_t G_s[i,i]
        for s in range(2):
            for t in range(2):
                assert numpy.max(numpy.abs(c[2 * s + t].sum(axis=1) - (na, nb)[t] * numpy.diag(G[s]))) < 1e-12


# ---------------------------------------------------------------- 3. translation_average
def test_translation_average_on_a_2x3_lattice():
    nx, ny = 2, 3                                   # sites i = ix + 2 iy: (0,0) (1,0) (0,1) (1,1) (0,2) (1,2)
    M = nx * ny
    c = numpy.arange(M * M, dtype=float).reshape(M, M)
    out = translation_average(c, nx, ny)
    assert out.shape == (ny, nx)
    assert out[0, 0] == numpy.mean(numpy.diag(c))
    # r = (rx, ry) = (1, 0): 0 -> 1, 1 -> 0, 2 -> 3, 3 -> 2, 4 -> 5, 5 -> 4
    assert out[0, 1] == numpy.mean([c[0, 1], c[1, 0], c[2, 3], c[3, 2], c[4, 5], c[5, 4]])
    # r = (0, 1): 0 -> 2, 1 -> 3, 2 -> 4, 3 -> 5, 4 -> 0, 5 -> 1
    assert out[1, 0] == numpy.mean([c[0, 2], c[1, 3], c[2, 4], c[3, 5], c[4, 0], c[5, 1]])
    # r = (1, 2): 0 -> 5, 1 -> 4, 2 -> 1, 3 -> 0, 4 -> 3, 5 -> 2
    assert out[2, 1] == numpy.mean([c[0, 5], c[1, 4], c[2, 1], c[3, 0], c[4, 3], c[5, 2]])
    # a translation-invariant function comes back as itself, on the Hubbard lattice's own ordering
    s = systems.Hubbard(nx, ny, 1, 1, 4.0)
    hop = translation_average(s.T[0], nx, ny)
    assert hop[0, 0] == 0 and hop[0, 1] == -2.0 and hop[1, 0] == hop[2, 0] == -1.0 and hop[1, 1] == 0
    with pytest.raises(ValueError):
        translation_average(c, 3, 3)


# ---------------------------------------------------------------- 4. the façade
@pytest.mark.parametrize("system", [generic, ueg, lambda: systems.Hubbard(4, 4, 7, 7, 4.0)])
def test_back_propagation_accepts_correlation(system):
    s = system()
    M = s.nbasis
    est = make_bp({'two_rdm': 'correlation'}, s)
    assert est.correlation and not est.structure_factor and est.two_rdm == []
    assert est.two_rdm_shape == (5, M, M)
    assert est.estimates.size == 3 + 1 + 2 * M * M + 5 * M * M
    assert make_bp({'two_rdm': 'correlation', 'evaluate_energy': True}, s).estimates.size == est.estimates.size


@pytest.mark.parametrize("one_rdm", [True, False])
def test_back_propagation_slicing_with_ekt(one_rdm):
    """The [5, M, M] block sits where the other two_rdm forms sit; the Fock matrices follow it."""
    s = generic()
    M = s.nbasis
    est = make_bp({'two_rdm': 'correlation', 'evaluate_ekt': True, 'one_rdm': one_rdm}, s)
    assert est.estimates.size == 3 + 1 + 2 * M * M + 5 * M * M + 2 * M * M
    est.estimates[:] = numpy.arange(est.estimates.size) + 0.5j
    est.accumulated = True
    est.buff_ix = 5
    flat = est.estimates.copy()
    est.print_step(Comm(), 1, 0)
    start = 4 + 2 * M * M
    assert est.two_rdm[0].shape == (5, M, M) and est.two_rdm[0].dtype == numpy.complex128
    assert numpy.array_equal(est.two_rdm[0].ravel(), flat[start:start + 5 * M * M])
    fock = 4 + (2 * M * M if one_rdm else 0) + 5 * M * M          # the reference's slicing (back_propagation.py:310-324)
    assert numpy.array_equal(est.fock_1p[0].ravel(), flat[fock:fock + M * M])
    assert numpy.array_equal(est.fock_1h[0].ravel(), flat[fock + M * M:fock + 2 * M * M])


def test_back_propagation_refusals():
    with pytest.raises(NotImplementedError):
        BackPropagation({'tau_bp': 0.025, 'two_rdm': 'correlation'}, True, None, QMC, generic(),
                        types.SimpleNamespace(ndets=3), complex, None)
    with pytest.raises(ValueError):
        make_bp({'two_rdm': 'correlations'}, generic())
    # the existing refusals stay
    for s in (generic(), systems.Hubbard(4, 4, 7, 7, 4.0)):
        with pytest.raises(NotImplementedError):
            make_bp({'two_rdm': 'structure_factor'}, s)
