"""The numpy restatement of the ITCF (tests/itcf_ref.py) against the genuine reference (make_golden_itcf.py): its
building blocks, and the window semantics it shares with the back-propagated estimator on recorded driver windows
(psi_R(0) = phi_old, the backward pass with its re-orthogonalisation, the weight factors, which walkers count)."""
import numpy
import pytest

from tests import itcf_ref


def close(a, b, tol=1e-12):
    a, b = numpy.asarray(a), numpy.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = float(numpy.max(numpy.abs(a - b))) / max(1.0, float(numpy.max(numpy.abs(b))))
    assert err <= tol, err


def test_generic_propagator_matrices(golden):
    d = golden('itcf_blocks.npz')
    for x, B in zip(d['g_fields'], d['g_B']):
        close(itcf_ref.b_generic(d['g_hs_pot'], d['g_BT2'], x, float(d['g_dt'])), B)


def test_hubbard_propagator_matrices(golden):
    d = golden('itcf_blocks.npz')
    for x, B in zip(d['h_fields'], d['h_B']):
        close(itcf_ref.b_hirsch(d['h_BT2'], x, float(d['h_dt']), float(d['h_U'])), B)


def test_back_propagation_with_store(golden):
    """back_propagate_generic(..., store=True) keeps phi after every step, most recent field first."""
    d = golden('itcf_blocks.npz')
    Bs = numpy.array([itcf_ref.b_generic(d['g_hs_pot'], d['g_BT2'], x, float(d['g_dt'])) for x in d['g_fields']])
    na = int(d['g_nelec'][0])
    psiL = itcf_ref.back_propagate(Bs, d['g_bp_phi'], na, int(d['g_bp_nstblz']))
    n = len(Bs)
    store = d['g_bp_store']
    assert len(store) == n
    for i in range(n):
        close(numpy.hstack(psiL[n - 1 - i]), store[i])


def test_gab_and_reortho(golden):
    d = golden('itcf_blocks.npz')
    close(itcf_ref.gab(d['gab_A'], d['gab_B']), d['gab'])
    close(itcf_ref.reortho(d['reortho_in']), d['reortho_Q'])


@pytest.mark.parametrize("tag", ['g_', 'h_'])
def test_recorded_driver_window(golden, tag):
    """Gls(0) = P(0) = gab(psi_L(0), psi_R(0)) of every walker, weighted like the ITCF, is the reference's
    back-propagated one-body RDM sum of the same window (G_bp = P^T), and the weights sum to its denominator."""
    d = golden('itcf_windows.npz')
    g = lambda k: d[tag + k]
    psi, BT2, dt, nstblz = g('psi'), g('BT2'), float(g('dt')), int(g('nstblz'))
    na = {'g_': 3, 'h_': 7}[tag]
    restore = str(g('restore'))
    wfac = g('weight').astype(complex)
    if restore == 'full':
        wfac = wfac * g('ph') / g('cos')
    else:
        assert restore == ''
    wins = []
    for w, fields in enumerate(g('fields')):
        if tag == 'g_':
            Bs = numpy.array([itcf_ref.b_generic(g('hs_pot'), BT2, x, dt) for x in fields])
        else:
            Bs = numpy.array([itcf_ref.b_hirsch(BT2, x, dt, float(g('U'))) for x in fields])
        wins.append(itcf_ref.window(Bs, g('phi_old')[w], psi, na, 1, nstblz) if wfac[w] != 0 else None)
    spgf = itcf_ref.accumulate(wins, wfac)
    close(numpy.sum(wfac), g('denom'))
    # the ITCF sums Re(wfac G) only for real wfac: compare the complex sum of P(0)^T directly
    P0 = sum(wt * numpy.array([win[1][0, s].T for s in range(2)]) for win, wt in zip(wins, wfac) if wt != 0)
    close(P0, g('G_sum'), 1e-10)
    if restore == '':
        close(spgf[0, :, 1], g('G_sum').transpose(0, 2, 1).real, 1e-10)
