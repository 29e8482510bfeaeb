"""Back-propagated UEG / Hubbard energies and the UEG structure factor, host side: the numpy restatement of the pair sums
against the reference's local_energy_ueg (ueg_sf_direct.npz), the index lists of UEG(full_lists=...), the estimator
classes' layout with the new options, and the refusals that remain.  No GPU."""
import types

import numpy
import pytest

from pauxy_amd import systems
from pauxy_amd.estimators.back_propagation import BackPropagation
from pauxy_amd.estimators.mixed import Mixed
from tests import ueg_sf_ref

CASES = ('u', 'p', 'c')


def rel(a, b):
    return float(numpy.max(numpy.abs(numpy.asarray(a) - numpy.asarray(b)))) / max(1.0, float(numpy.max(numpy.abs(b))))


def system_of(d, tag, full):
    rs, nup, ndown, ecut = d[tag + '_sys']
    return systems.UEG(float(rs), int(nup), int(ndown), float(ecut), full_lists=full)


@pytest.mark.parametrize("tag", CASES)
@pytest.mark.parametrize("full", [False, True])
def test_restatement_is_the_reference(golden, tag, full):
    d = golden('ueg_sf_direct.npz')
    s = system_of(d, tag, full)
    key = tag + ('f' if full else 't') + '_'
    assert len(d[tag + '_G']) >= 2
    for G, E, two in zip(d[tag + '_G'], d[key + 'E'], d[key + 'two_rdm']):
        e, t = ueg_sf_ref.evaluate(s, G)
        assert t.shape == two.shape == (2, 2, len(s.qvecs))
        assert rel(t, two) < 1e-13
        assert rel(e, E) < 1e-13


@pytest.mark.parametrize("tag", CASES)
def test_full_lists_are_the_reference_thermal_lists(golden, tag):
    d = golden('ueg_sf_direct.npz')
    s = system_of(d, tag, True)
    for nm in ('ikpq_i', 'ikpq_kpq', 'ipmq_i', 'ipmq_pmq'):
        want = ueg_sf_ref.ragged(d, tag + 'f_' + nm)
        got = getattr(s, nm)
        assert len(got) == len(want) == len(s.qvecs)
        for a, b in zip(got, want):
            assert numpy.array_equal(a, b)


def test_default_lists_unchanged(golden):
    """The default stays the reference's: first nup plane waves, the lists traj_ueg.npz recorded."""
    from tests.helpers import ragged
    d = golden('traj_ueg.npz')
    s = systems.UEG(float(d['sys_rs']), 7, 7, float(d['sys_ecut']))
    assert not s.full_lists
    for nm in ('ikpq_i', 'ikpq_kpq', 'ipmq_i', 'ipmq_pmq'):
        want = ragged(d, nm, 'sys_')
        for a, b in zip(getattr(s, nm), want):
            assert numpy.array_equal(a, b)
        assert max(len(x) for x in getattr(s, nm)) <= 7
    f = systems.UEG(float(d['sys_rs']), 7, 7, float(d['sys_ecut']), full_lists=True)
    assert max(len(x) for x in f.ikpq_i) > 7 and all(numpy.all(x < f.nbasis) for x in f.ikpq_i)
    # everything but the lists is the same system
    assert numpy.array_equal(f.vqvec, s.vqvec) and f.nbasis == s.nbasis and (f.iA != s.iA).nnz == 0


def test_truncated_and_full_lists_differ_on_dense_rows(golden):
    """The third fact of the issue: on a back-propagated Green's function the truncated lists leave part of the sums
    out (on the mixed Green's function of the Hartree-Fock trial they do not)."""
    d = golden('ueg_sf_direct.npz')
    G = d['u_G'][0]
    assert rel(d['ut_two_rdm'][0], d['uf_two_rdm'][0]) > 1e-3
    s, f = system_of(d, 'u', False), system_of(d, 'u', True)
    Gm = numpy.zeros_like(G)
    Gm[0, :7, :7] = numpy.eye(7)
    Gm[1, :7, :7] = numpy.eye(7)
    assert rel(ueg_sf_ref.evaluate(s, Gm)[1], ueg_sf_ref.evaluate(f, Gm)[1]) == 0.0


# ---------------------------------------------------------------- estimator classes
QMC = types.SimpleNamespace(dt=0.005, nstblz=5, nsteps=10)
TRIAL = types.SimpleNamespace(ndets=1)


def ueg():
    return systems.UEG(2.0, 7, 7, 1.0)


def generic(M=5, K=6):
    rng = numpy.random.RandomState(1)
    h = rng.normal(size=(M, M))
    A = rng.normal(size=(K, M, M))
    Lv = 0.5 * (A + A.transpose(0, 2, 1))
    return systems.Generic((2, 2), numpy.array([h + h.T, h + h.T]), numpy.ascontiguousarray(Lv.reshape(K, M * M).T))


def make_bp(bp, system):
    return BackPropagation(dict(bp, tau_bp=0.025), True, None, QMC, system, TRIAL, complex, None)


class Comm(object):
    rank = 0
    size = 1

    def Reduce(self, a, b, op=None, root=0):
        b[:] = a

    def bcast(self, x, root=0):
        return x


def test_back_propagation_accepts_the_options():
    s = ueg()
    M, nq = s.nbasis, len(s.qvecs)
    est = make_bp({'evaluate_energy': True, 'two_rdm': 'structure_factor'}, s)
    assert est.eval_energy and est.structure_factor and est.two_rdm == []
    assert est.two_rdm_shape == (2, 2, nq)
    assert est.estimates.size == 3 + 1 + 2 * M * M + 4 * nq                  # back_propagation.py:84-106
    # also without the energies, and the energies on all three systems
    assert make_bp({'two_rdm': 'structure_factor'}, s).estimates.size == 3 + 1 + 2 * M * M + 4 * nq
    assert make_bp({'evaluate_energy': True}, systems.Hubbard(4, 4, 7, 7, 4.0)).eval_energy
    assert make_bp({'evaluate_energy': True}, generic()).eval_energy
    # the M^4 two-body RDM keeps its layout
    assert make_bp({'two_rdm': True}, s).two_rdm_shape == (M,) * 4


@pytest.mark.parametrize("one_rdm", [True, False])
def test_back_propagation_slicing(one_rdm):
    """back_propagation.py:290-306: energies / weight, the one-body RDM, then the [2, 2, nq] block."""
    s = ueg()
    M, nq = s.nbasis, len(s.qvecs)
    est = make_bp({'evaluate_energy': True, 'two_rdm': 'structure_factor', 'one_rdm': one_rdm}, s)
    est.estimates[:] = numpy.arange(est.estimates.size) + 0.5j
    est.accumulated = True
    est.buff_ix = 5
    flat = est.estimates.copy()
    est.print_step(Comm(), 1, 0)
    assert numpy.array_equal(est.energies[0], flat[:3] / flat[3])
    assert est.denominator[0] == flat[3]
    assert len(est.one_rdm) == (1 if one_rdm else 0)
    start = 4 + 2 * M * M
    assert est.two_rdm[0].shape == (2, 2, nq) and est.two_rdm[0].dtype == numpy.complex128
    assert numpy.array_equal(est.two_rdm[0].ravel(), flat[start:start + 4 * nq])


def test_back_propagation_refusals():
    for s in (generic(), systems.Hubbard(4, 4, 7, 7, 4.0)):
        with pytest.raises(NotImplementedError):
            make_bp({'two_rdm': 'structure_factor'}, s)
    with pytest.raises(ValueError):
        make_bp({'two_rdm': 'structure'}, ueg())
    with pytest.raises(NotImplementedError):                 # multi-determinant windows stay on Generic systems
        BackPropagation({'tau_bp': 0.025, 'evaluate_energy': True}, True, None, QMC, ueg(),
                        types.SimpleNamespace(ndets=2), complex, None)


def make_mixed(opts, system):
    return Mixed(dict(opts, verbose=False), system, True, None, QMC, TRIAL)


def test_mixed_accepts_the_structure_factor():
    s = ueg()
    nq = len(s.qvecs)
    est = make_mixed({'two_rdm': 'structure_factor'}, s)
    assert est.structure_factor and est.sf_acc.shape == (2, 2, nq) and est.two_rdm == []
    off = make_mixed({}, s)
    assert not off.structure_factor and 'two_rdm' not in off.__dict__ and 'sf_acc' not in off.__dict__


def test_mixed_block_is_the_accumulator_over_the_energy_denominator():
    s = ueg()
    est = make_mixed({'two_rdm': 'structure_factor'}, s)
    ns = est.names
    est.estimates[ns.weight] = 20.0
    est.estimates[ns.edenom] = 4.0
    est.estimates[ns.enumer] = 8.0
    est.sf_acc[:] = numpy.arange(est.sf_acc.size).reshape(est.sf_acc.shape)
    want = est.sf_acc / 4.0
    est.print_step(Comm(), 1, 10)
    assert len(est.two_rdm) == 1 and numpy.array_equal(est.two_rdm[0], want)
    assert est.two_rdm[0].dtype == numpy.float64
    assert not est.sf_acc.any()                              # zeroed for the next block


def test_mixed_refusals():
    with pytest.raises(NotImplementedError):
        make_mixed({'two_rdm': True}, ueg())
    for s in (generic(), systems.Hubbard(4, 4, 7, 7, 4.0)):
        with pytest.raises(NotImplementedError):
            make_mixed({'two_rdm': 'structure_factor'}, s)
    est = make_mixed({'two_rdm': 'structure_factor'}, ueg())
    with pytest.raises(NotImplementedError):
        est.update(ueg(), QMC, TRIAL, None, 0, free_projection=True)


def test_golden_trajectory_fixtures(golden):
    d = golden('ueg_sf_traj.npz')
    n = len(golden('traj_bp_ueg.npz')['bp_denominator'])
    assert d['bp_energies'].shape == (n, 3) and d['bp_two_rdm'].shape == (n, 2, 2, 256)
    assert numpy.all(numpy.isfinite(d['bp_two_rdm'])) and numpy.abs(d['bp_two_rdm']).max() > 1.0
    h = golden('hubbard_bp_energy.npz')
    assert h['bp_energies'].shape == (len(golden('traj_hirsch_bp.npz')['bp_denominator']), 3)
    # E = E1b + E2b in every window
    for e in (d['bp_energies'], h['bp_energies']):
        assert rel(e[:, 0], e[:, 1] + e[:, 2]) < 1e-13
