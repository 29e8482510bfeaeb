"""The table of tests/between_steps_cases.py, where there is no GPU: that it names every entry point of the header, and
that the harness agrees with itself -- the same cases driven over the numpy stand-in (tests/oracle_device.OracleDevice)
meet the oracle steps built from the state read back behind the event.  The stand-in caches nothing, so this pins what the
harness expects of a revived walker, of an uploaded overlap, of a comb and of a changed model to the oracle's own behaviour
before any device time is spent.

Tolerance: both sides run the oracle's statements on the same numbers, one through the stand-in's walker dicts and one
through walkers rebuilt from the read-back arrays, so they are two orderings of the same fp64 arithmetic.  Measured over
every row below: the largest deviation of any field is 0.0 (the same bits).  Ten times that is still zero, so the bound is one
unit in the last place of the field's largest element, 2.3e-16 relative -- anything more is a harness that models an
event wrongly."""
import os
import re

import numpy
import pytest

from pauxy_amd import _lib as L
from tests import between_steps_cases as bs
from tests.oracle_device import OracleDevice

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 2.3e-16


def declared_entry_points():
    text = open(os.path.join(HERE, '..', 'include', 'afqmc_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    return sorted(set(re.findall(r'\b(afq_[a-z0-9_]+)\s*\(', text)))


def test_every_entry_point_is_a_row_or_exempt_with_a_reason():
    names = declared_entry_points()
    assert len(names) > 100 and 'afq_walkers_set' in names and 'afq_popcontrol_comb_local' in names
    rows = set(c for r in bs.ROWS for c in r.calls)
    thermal = set(n for n in names if n.startswith('afq_thermal_'))      # finite-temperature walkers: another walk, no phi
    unclassified = [n for n in names if n not in rows and n not in bs.EXEMPT and n not in thermal]
    assert unclassified == [], unclassified
    stale = sorted((rows | set(bs.EXEMPT)) - set(names))
    assert stale == [], stale                                            # a row about an entry point that is gone
    both = sorted(rows & set(bs.EXEMPT))
    assert both == [], both
    assert all(isinstance(why, str) and why for why in bs.EXEMPT.values())


def test_the_table_is_well_formed():
    assert len(bs.ROW) == len(bs.ROWS)
    for r in bs.ROWS:
        assert r.kind in ('writer', 'reader', 'config') and r.hands in ('still', 'on', 'off', None), r.name
        assert any(r.runs_on(c) for c in bs.CONFIGS), r.name
        if r.kind == 'reader':
            assert r.moves == (), r.name
    ids = ["%s-%s-%s" % c for c in bs.cases()]
    assert len(set(ids)) == len(ids)
    for c in bs.CONFIGS:
        assert any(i.startswith(c + '-') for i in ids)


def make_stand_in(model, nw):
    dev = OracleDevice()
    assert model.kind == 'generic'
    dev.set_system_generic(model.hs_pot, model.rchol, model.H1, model.ecore, model.na, model.nb)
    dev.set_trial(model.psi)
    bs.upload_propagator(dev, model)
    dev.walkers_alloc(nw)
    return dev


def deviation(a, b):
    a, b = numpy.asarray(a), numpy.asarray(b)
    return float(numpy.abs(a - b).max()) / max(1.0, float(numpy.abs(b).max()))


ORACLE_ROWS = [r.name for r in bs.ROWS if r.oracle and r.runs_on('rhf24')]


def test_the_stand_in_covers_the_rows_the_issue_names():
    want = {'set_phi_swap', 'set_phi_one', 'set_phi_open', 'set_ghalf_garbage', 'set_ot_scaled', 'set_weight_revive_kill',
            'reset_weights', 'reortho', 'copy_closed_closed', 'copy_open_closed', 'copy_closed_open', 'copy_live_dead',
            'popcontrol_comb', 'scale_weights', 'cap_weights', 'set_weight_cap', 'greens', 'force_bias', 'local_energy',
            'estimates_update', 'estimates_update_energy', 'get_ghalf', 'bp_update', 'set_system',
            'set_propagator_dt', 'set_propagator_same', 'set_propagator_order', 'set_trial_real_closed', 'set_trial_complex'}
    assert want <= set(ORACLE_ROWS), want - set(ORACLE_ROWS)


@pytest.mark.parametrize("warm", ['full', 'energy'])
@pytest.mark.parametrize("name", ORACLE_ROWS)
def test_harness_against_the_stand_in(name, warm):
    """rhf24 (M = 24, K = 30, 5 + 5, 24 walkers, one open-shell and one dead): the teeth of the row hold on the stand-in
    too, and the two steps behind the event, Ghalf and the energies meet the oracle of the read-back state."""
    out = bs.run_case('rhf24', warm, name, make_stand_in)
    r = bs.ROW[name]
    bs.check_teeth(r, out)
    worst = 0.0
    for got, want in out['steps']:
        for i in range(len(want['live'])):
            if not bs.is_live(out['after'][L.F_WEIGHT][i]):
                assert bs.same_bits(got[L.F_PHI][i], out['after'][L.F_PHI][i]) and got[L.F_WEIGHT][i] == out['after'][L.F_WEIGHT][i]
                continue
            for f, key in ((L.F_PHI, 'phi'), (L.F_WEIGHT, 'weight'), (L.F_OT, 'ot'), (L.F_HYBRID_ENERGY, 'ehyb'), (L.F_PHASE, 'phase')):
                worst = max(worst, deviation(got[f][i], want[key][i]))
    last = out['steps'][-1][1]
    for i in range(len(last['live'])):                                   # Ghalf and the energies behind the second step
        if bs.is_live(out['after'][L.F_WEIGHT][i]) and bs.is_live(last['weight'][i]):
            worst = max(worst, deviation(out['ghalf'][i], out['want_ghalf'][i]), deviation(out['energy'][i], out['want_energy'][i]))
    print('%s %s: largest deviation %.3e' % (name, warm, worst))
    assert worst <= TOL, worst
