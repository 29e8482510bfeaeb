"""The direct update, the free projection and the back-propagation of the discrete Hirsch fields (csrc/k_hirsch.hip:
hirsch_direct_*, hirsch_free_*, bp_hirsch_*) against the oracle, call by call, on the lattices of tests/hirsch_path_cases.py:
both sides of the 32 / 45-electron limits of the inverse overlaps, unequal and empty spins, the second (ragged) chunk of 256
sites of the direct update, the one-body products of 64 walkers with dead ones among them, both decompositions, the kill
branch of the direct update, walkers the kinetic step killed, the use_log_shift factors, and windows whose walkers hold
histories of different lengths.  The golden trajectories replay these paths on a 4 x 4 lattice only.

Chosen fields, ``used``, exact-zero weights and everything about a walker that must not be touched are compared exactly.
phi and G are compared in the measure of ``run_hirsch_lattice`` (largest difference over max(1, largest reference value)),
weight, ot and phase walker by walker relative to the reference value, with the bounds below; every comparison prints its
error (-s), profiles/hirsch_paths_precision.md keeps the largest per case."""
import numpy
import pytest

from pauxy_amd import _lib as L
from pauxy_amd.device import AfqDevice
from tests import hirsch_path_cases as hc
from tests.philox_ref import MASK, W0, philox4x32_10_vec

pytestmark = pytest.mark.gpu

# Ceilings: what run_hirsch_lattice asks of the single-site update (phi 1e-9, weight and ot 1e-8; the phase, a product of
# unit factors made by sincos, gets the bound of phi) and test_back_propagation_with_reortho of a window (denominator 1e-9,
# G 1e-8).  The largest errors measured over all cases (profiles/hirsch_paths_precision.md) are phi 7.8e-16, weight 5.2e-14,
# ot 1.6e-14, phase 4.9e-16, denominator 1.2e-15, G 1.9e-15: orders of magnitude below, so the bounds are 100 times the
# measured values, and no less than 100 x 1e-15.
TOL = dict(phi=1e-13, weight=5.2e-12, ot=1.6e-12, phase=1e-13, denominator=1.2e-13, G=1.9e-13)


def check(case, path, quantity, got, want):
    """phi, G and the denominator in the measure of run_hirsch_lattice; the per-walker scalars relative to the walker's own
    value, which asks more: the charge decomposition's direct update leaves weights of order 2^-M, and a measure relative to
    max(1, .) would compare nothing there.  An exact zero of the oracle must be an exact zero."""
    got, want = numpy.asarray(got), numpy.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if quantity in ('weight', 'ot', 'phase'):
        nz = want != 0
        assert numpy.all(got[~nz] == 0), (case, path, quantity)
        err = float(numpy.max(numpy.abs(got[nz] - want[nz]) / numpy.abs(want[nz]), initial=0.0))
    else:
        err = float(numpy.max(numpy.abs(got - want))) / max(1.0, float(numpy.max(numpy.abs(want))))
    print("PRECISION | %s | %s | %s | %.1e | %.1e" % (case, path, quantity, err, TOL[quantity]))
    assert err <= TOL[quantity], (case, path, quantity, err)


def device_for(m, nw, charge, phis, weights, ot):
    dev = AfqDevice(0)
    dev.set_system_hubbard(m.H1, m.U, m.na, m.nb)
    dev.set_trial(m.psi)
    dev.set_propagator_hirsch(m.bt2, m.dt, charge)
    dev.walkers_alloc(nw)
    if getattr(m, 'log_shift', 0.0):
        dev.set_log_shift(True, m.log_shift)
    dev.set(L.F_PHI, phis)
    dev.set(L.F_WEIGHT, weights)
    dev.set(L.F_OT, ot)
    return dev


def state(dev):
    return dict(phi=dev.get(L.F_PHI), weight=dev.get(L.F_WEIGHT), ot=dev.get(L.F_OT), phase=dev.get(L.F_PHASE))


def compare(case, path, got, want, walkers, quantities=('phi', 'weight', 'ot')):
    for q in quantities:
        check(case, path, q, got[q][walkers], want[q][walkers])
    zero = want['weight'] == 0.0
    assert numpy.all(got['weight'][zero] == 0.0) and numpy.all(got['weight'][~zero] != 0.0)


def same(a, b, walker, quantities=('phi', 'weight', 'ot')):
    return all(numpy.array_equal(a[q][walker], b[q][walker]) for q in quantities)


@pytest.mark.parametrize("name", sorted(hc.DIRECT))
def test_direct_update_step_by_step(name):
    """``single_site_update: False``: kinetic step, two_body_direct (hubbard.py:222-275), second kinetic step and energy
    shift, every walker against the oracle after each call."""
    run = hc.run_direct(name)
    m, phis, w0, ot0, u = run['case']
    spec = hc.DIRECT[name]
    nw, M = spec['nw'], m.M
    everyone = numpy.arange(nw)
    dev = device_for(m, nw, spec['charge'], phis, w0, ot0)
    dev.hirsch_single_site(False)
    start = state(dev)
    assert same(start, dict(phi=phis, weight=w0, ot=ot0), everyone)
    # ---- kinetic step: kills the walker that tracks minus its overlap, and leaves its ot alone
    dev.hirsch_kinetic()
    kin = state(dev)
    compare(name, 'direct: kinetic', kin, run['kinetic'], everyone)
    assert kin['weight'][hc.FLIPPED] == 0.0 and kin['ot'][hc.FLIPPED] == ot0[hc.FLIPPED]
    assert same(kin, start, hc.DEAD)
    # ---- the direct update
    fields, used = dev.hirsch_two_body(u)
    two = state(dev)
    assert numpy.array_equal(fields, run['fields']) and numpy.array_equal(used, run['used'])
    updated = run['used'] == M
    assert numpy.all(fields[~updated] == -1) and numpy.all(used[~updated] == 0) and updated.sum() >= 1
    compare(name, 'direct: two_body', two, run['two_body'], everyone)
    assert same(two, start, hc.DEAD) and same(two, kin, hc.FLIPPED)
    if 'kill' in spec:                                     # |arg(wfac ovlp / ot)| >= pi / 2: weight 0, ot as it was
        k = spec['kill']
        assert updated[k] and kin['weight'][k] != 0.0 and two['weight'][k] == 0.0 and two['ot'][k] == kin['ot'][k]
        assert numpy.count_nonzero(two['weight'][updated]) == updated.sum() - 1
    # ---- second kinetic step, exp(dt eshift)
    dev.hirsch_finish(hc.ESHIFT)
    fin = state(dev)
    compare(name, 'direct: finish', fin, run['finish'], everyone)
    assert same(fin, start, hc.DEAD) and same(fin, kin, hc.FLIPPED)
    if 'kill' in spec:
        assert same(fin, two, spec['kill'])
    dev.close()


def device_uniforms(n, seed, stream, counter):
    """rng_uniform_kernel restated: pair p uses the counter words of the normals' stream (tests/philox_ref.py), the top 53
    bits of c0:c1 and of c2:c3 are the two uniforms in [0, 1)."""
    p = numpy.arange((n + 1) // 2, dtype=numpy.uint64)
    m32, s32 = numpy.uint64(MASK), numpy.uint64(32)
    c = philox4x32_10_vec(p & m32, (p >> s32) & m32, numpy.uint64(counter & MASK),
                          numpy.uint64(((counter >> 32) ^ (stream * W0)) & MASK), seed & MASK, (seed >> 32) & MASK)
    out = numpy.empty(2 * len(p))
    out[0::2] = (((c[0] << s32) | c[1]) >> numpy.uint64(11)).astype(numpy.float64) / 9007199254740992.0
    out[1::2] = (((c[2] << s32) | c[3]) >> numpy.uint64(11)).astype(numpy.float64) / 9007199254740992.0
    return out[:n]


@pytest.mark.parametrize("name", sorted(hc.FREE))
def test_free_projection_step_by_step(name):
    """propagate_walker_free (hubbard.py:303-343), two steps -- the second starts from the device's own ot and phase; the
    walkers with |weight| <= 1e-8 come back bit for bit.  Then one step on the device's own uniforms: the fields are
    ``u < 0.5`` of the stream restated from the Philox counters."""
    run = hc.run_free(name)
    m, phis, w0, ot0, u = run['case']
    spec = hc.FREE[name]
    nw, M = spec['nw'], m.M
    live = numpy.abs(w0) > 1e-8
    dev = device_for(m, nw, spec['charge'], phis, w0, ot0)
    with pytest.raises(L.AfqError) as e:
        dev.propagate_hirsch_free(u[0], hc.ESHIFT)
    assert e.value.code == L.AFQ_ESTATE and 'afq_hirsch_free_projection(h, 1) first' in str(e.value)
    dev.hirsch_free_projection(True)
    start = state(dev)
    for n, (us, want) in enumerate(zip(u, run['steps'])):
        fields = dev.propagate_hirsch_free(us, hc.ESHIFT, fetch_fields=True)
        got = state(dev)
        assert numpy.array_equal(fields, want['fields'])
        assert numpy.all(fields[~live] == -1) and numpy.all(fields[live] >= 0)
        compare(name, 'free: step %d' % (n + 1), got, want, numpy.arange(nw), ('phi', 'weight', 'ot', 'phase'))
        for i in numpy.nonzero(~live)[0]:
            assert same(got, start, i, ('phi', 'weight', 'ot', 'phase'))
    before = state(dev)
    seed, stream = 0x0123456789ABCDEF, 3
    dev.rng_seed(seed, stream)
    fields = dev.propagate_hirsch_free(None, hc.ESHIFT, fetch_fields=True)
    want = numpy.where(device_uniforms(nw * M, seed, stream, 0).reshape(nw, M) < 0.5, 0, 1)
    assert numpy.array_equal(fields[live], want[live]) and numpy.all(fields[~live] == -1)
    after = state(dev)
    for i in numpy.nonzero(~live)[0]:
        assert same(after, before, i, ('phi', 'weight', 'ot', 'phase'))
    assert not any(numpy.array_equal(after['phi'][i], before['phi'][i]) for i in numpy.nonzero(live)[0])
    dev.close()


@pytest.mark.parametrize("name", sorted(hc.BP))
def test_back_propagation_of_discrete_fields(name):
    """afq_bp_update (propagation/hubbard.py:568-672, estimators/back_propagation.py:127-226) after windows of single-site
    steps: the spin decomposition's factors on the recorded fields whatever propagated them, most recent configuration
    first, re-orthogonalised inside the window, with a walker copied in mid-window (its history travels), walkers that stay
    dead, and one given a weight in mid-window: its history is shorter, and it counts."""
    run = hc.run_bp(name)
    m, phis, w0, ot0, u, spec = run['case']
    nw, M, nbp = spec['nw'], m.M, spec['nbp']
    # the fixture, on the oracle alone (tests/test_hirsch_paths_cpu.py leaves the 64-walker window to this test)
    first, second = run['steps']
    assert first[hc.SRC] == first[hc.DST] == nbp and 0 < first[hc.DEAD] == nbp - 1 - spec['revive_after'] < nbp
    assert run['weights'][nbp - 1][hc.DEAD] > 1e-8 and numpy.count_nonzero(first == 0) >= 1
    dev = device_for(m, nw, spec['charge'], phis, w0, ot0)
    dev.bp_configure(nbp)
    with pytest.raises(L.AfqError) as e:
        dev.hirsch_single_site(False)
    assert e.value.code == L.AFQ_EUNSUPPORTED and 'the direct Hirsch update records no field history' in str(e.value)
    with pytest.raises(L.AfqError) as e:
        dev.hirsch_free_projection(True)
    assert e.value.code == L.AFQ_EUNSUPPORTED and 'no field history in free projection' in str(e.value)
    assert list(dev.bp_steps()) == [0] * nw
    step = 0
    for window, n in enumerate((nbp, spec['nbp2'])):
        for k in range(n):
            dev.hirsch_kinetic()
            fields, used = dev.hirsch_two_body(u[step])
            dev.hirsch_finish(hc.ESHIFT)
            assert numpy.array_equal(fields, run['fields'][step]), step
            check(name, 'bp: window %d' % (window + 1), 'weight', dev.get(L.F_WEIGHT), run['weights'][step])
            step += 1
            if window == 0 and k == spec['revive_after']:
                dev.set(L.F_WEIGHT, numpy.array([hc.REVIVED_WEIGHT]), first=hc.DEAD)
            if window == 0 and k == spec['copy_after']:
                dev.copy_walker(hc.SRC, hc.DST)
        assert numpy.array_equal(dev.bp_steps(), run['steps'][window])
        est = run['est'][window]
        energies, denom, G = dev.bp_update(m.psi, spec['nstblz'], None)
        check(name, 'bp: window %d' % (window + 1), 'denominator', denom, est[3])
        check(name, 'bp: window %d' % (window + 1), 'G', G, est[4:].reshape(2, M, M))
        assert numpy.all(energies == 0) and list(dev.bp_steps()) == [0] * nw
    dev.close()


def test_direct_and_free_refuse_a_configured_window():
    """The other order: the direct update chosen first, a window configured afterwards -- the update itself refuses; free
    projection first -- the window cannot be configured."""
    m, phis, w0, ot0, u = hc.build_direct('2x2-spin')
    dev = device_for(m, len(w0), False, phis, w0, ot0)
    dev.hirsch_single_site(False)
    dev.bp_configure(2)
    dev.hirsch_kinetic()
    with pytest.raises(L.AfqError) as e:
        dev.hirsch_two_body(u)
    assert e.value.code == L.AFQ_EUNSUPPORTED and 'the direct Hirsch update records no field history' in str(e.value)
    dev.close()
    dev = device_for(m, len(w0), False, phis, w0, ot0)
    dev.hirsch_free_projection(True)
    with pytest.raises(L.AfqError) as e:
        dev.bp_configure(2)
    assert e.value.code == L.AFQ_EUNSUPPORTED and 'no field history in free projection' in str(e.value)
    dev.close()
