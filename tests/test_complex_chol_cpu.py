"""Complex Cholesky vectors (afq_set_system_generic_c128): the C-ABI entry point exists and refuses a null handle,
the CPU oracle reproduces the genuine reference's complex-L fixtures (tests/golden/make_golden_cplx.py), and a complex
dense QMCPACK Hamiltonian reaches the system object complex.  CPU only."""
import ctypes
import os
import re

import numpy

from oracle import afqmc_ref as ref
from pauxy_amd import _lib
from tests.helpers import generic_model
from tests.test_oracle_golden import check_msd_steps, check_single_walker_ops, close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c128_entry_point_declared_exported_and_refuses_null():
    text = open(os.path.join(ROOT, "include", "afqmc_hip.h")).read()
    assert re.search(r"int afq_set_system_generic_c128\(afq_handle \*h, int M, int K, int na, int nb,", text)
    assert "afq_set_system_generic_c128" in _lib.SIGNATURES
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    one = numpy.zeros(8)
    p = one.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.afq_set_system_generic_c128(None, 2, 1, 1, 1, p, p, p, 0.0) == -1      # AFQ_EINVAL


def test_oracle_reproduces_complex_cholesky_fixtures(golden):
    d = golden('cplx_ops.npz')
    for tag, herm in (('H_', True), ('E_', True), ('N_', False)):
        chol = d[tag + 'chol']
        assert numpy.iscomplexobj(chol) and numpy.abs(chol.imag).max() > 0.1
        M = d[tag + 'h1e'].shape[0]
        L = chol.T.reshape(-1, M, M)
        assert numpy.array_equal(L, L.conj().transpose(0, 2, 1)) == herm
        model = generic_model(d, tag)
        check_single_walker_ops(d, tag, model)
        G = d[tag + 'G']
        close(numpy.array(ref.local_energy_generic_cholesky(model.H1, model.ecore, G, chol)), d[tag + 'energy_full'])
    assert 'E_step_phi' in d and 'N_step_phi' in d


def test_oracle_reproduces_complex_cholesky_nomsd_fixture(golden):
    """The reference's multi-determinant path runs with Hermitian complex L; the oracle reproduces its ten steps."""
    d = golden('msd_cplx.npz')
    M = d['h1e'].shape[0]
    L3 = d['chol'].T.reshape(-1, M, M)
    assert numpy.array_equal(L3, L3.conj().transpose(0, 2, 1)) and numpy.abs(L3.imag).max() > 0.1
    check_msd_steps(d, 'N_', True)


def test_complex_qmcpack_dense_hamiltonian_stays_complex(tmp_path):
    from pauxy_amd.systems import get_system
    from pauxy_amd.utils import io as aio
    rng = numpy.random.RandomState(5)
    M, K = 5, 6
    h = rng.normal(size=(M, M))
    h = 0.5 * (h + h.T)
    A = rng.normal(size=(K, M, M)) + 1j * rng.normal(size=(K, M, M))
    chol = (0.5 * (A + A.conj().transpose(0, 2, 1))).reshape(K, M * M).T.copy()
    path = str(tmp_path / 'ham.h5')
    aio.write_qmcpack_dense(h.astype(complex), chol, (2, 2), M, enuc=0.25, filename=path, real_chol=False)
    s = get_system({'name': 'Generic', 'integrals': path, 'nup': 2, 'ndown': 2})
    assert numpy.iscomplexobj(s.hs_pot) and numpy.array_equal(s.hs_pot, chol)
    # v0 = 1/2 sum_kn L[ik,n] L[jk,n] without conjugation (systems/generic.py:202-210)
    c3 = chol.reshape(M, M, K)
    v0 = 0.5 * numpy.einsum('ikn,jkn->ij', c3, c3)
    assert numpy.allclose(s.h1e_mod[0], s.H1[0] - v0, rtol=0, atol=1e-13)


def test_back_propagation_refuses_general_complex_cholesky():
    """The device back-propagation reuses the forward step with fields -conj(x): exact for Hermitian L only."""
    import pytest
    from types import SimpleNamespace
    from pauxy_amd.estimators.back_propagation import BackPropagation
    from pauxy_amd.systems import Generic
    rng = numpy.random.RandomState(2)
    M, K = 4, 3
    A = rng.normal(size=(K, M, M)) + 1j * rng.normal(size=(K, M, M))
    h1 = numpy.array([numpy.eye(M), numpy.eye(M)])
    qmc = SimpleNamespace(dt=0.01, nstblz=5)
    general = Generic((1, 1), h1, A.reshape(K, M * M).T.copy())
    with pytest.raises(NotImplementedError, match='Hermitian'):
        BackPropagation({'tau_bp': 0.05}, True, None, qmc, general, None, numpy.complex128, None)
    herm = Generic((1, 1), h1, (0.5 * (A + A.conj().transpose(0, 2, 1))).reshape(K, M * M).T.copy())
    try:
        BackPropagation({'tau_bp': 0.05}, True, None, qmc, herm, None, numpy.complex128, None)
    except NotImplementedError as e:
        raise AssertionError(e)
    except Exception:
        pass                  # (a later step of the set-up may want a real trial / propagator: not what is tested)
