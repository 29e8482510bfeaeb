"""Back-propagated UEG / Hubbard energies and the UEG structure factor on the device (k_ueg_sf.hip): trajectories of the
genuine reference replayed through both driver loops (make_golden_ueg_sf.py), the pair-sum kernel against the
reference's local_energy_ueg (ueg_sf_direct.npz) and against the numpy restatement (tests/ueg_sf_ref.py) on every
dispatch boundary it has, the window's weighted sums against per-walker G_bp put through the restatement, the mixed
accumulation against the walkers' Green's functions, and bitwise reproducibility.

Tolerance: `close` of tests/test_gpu_traj.py at 1e-8 (error relative to max(1, max|want|)), the bound
test_gpu_bp_obs.py uses for sums of the same kind."""
import numpy
import pytest

from pauxy_amd import _lib as L, systems, trial as trial_mod
from pauxy_amd.context import release_context
from pauxy_amd.device import AfqDevice
from pauxy_amd.estimators.mixed import local_energy
from pauxy_amd.propagation import setup
from pauxy_amd.qmc.afqmc import AFQMC
from pauxy_amd.utils.io import extract_rdm
from oracle import afqmc_ref as ref
from tests import ueg_sf_ref
from tests.helpers import make_device
from tests.test_gpu_bp_obs import capture_bp
from tests.test_gpu_traj import close, replay, run_hirsch

pytestmark = pytest.mark.gpu
TOL = 1e-8


# ---------------------------------------------------------------- 1. trajectories of the reference
@pytest.mark.parametrize("batched", [False, True])
def test_traj_ueg_energies_and_structure_factor(golden, monkeypatch, tmp_path, batched):
    d = dict(golden('traj_bp_ueg.npz'))
    want = golden('ueg_sf_traj.npz')
    s = systems.UEG(float(d['sys_rs']), 7, 7, float(d['sys_ecut']))
    t = trial_mod.hartree_fock_ueg(s)
    got = capture_bp(monkeypatch)
    bp = {'tau_bp': 0.04, 'one_rdm': True, 'evaluate_energy': True, 'two_rdm': 'structure_factor'}
    replay(d, s, t, {}, monkeypatch, est_extra={'back_propagated': bp, 'basename': str(tmp_path / 'estimates')},
           batched=batched)
    est = got['est']
    close(numpy.array(est.denominator), d['bp_denominator'])
    close(numpy.array(est.one_rdm), d['bp_one_rdm'])
    assert len(est.energies) == len(want['bp_energies']) == len(est.two_rdm)
    close(numpy.array(est.energies), want['bp_energies'])
    close(numpy.array(est.two_rdm), want['bp_two_rdm'])
    fn = str(tmp_path / 'estimates.0.h5')
    den = numpy.array(est.denominator)
    assert numpy.array_equal(extract_rdm(fn, rdm_type='two_rdm'), numpy.array(est.two_rdm) / den[:, None, None, None])


def test_traj_ueg_structure_factor_without_energies(golden, monkeypatch):
    """The deliberate difference: the structure factor is evaluated also with evaluate_energy: False."""
    d = dict(golden('traj_bp_ueg.npz'))
    want = golden('ueg_sf_traj.npz')
    s = systems.UEG(float(d['sys_rs']), 7, 7, float(d['sys_ecut']))
    t = trial_mod.hartree_fock_ueg(s)
    got = capture_bp(monkeypatch)
    replay(d, s, t, {}, monkeypatch, batched=True,
           est_extra={'back_propagated': {'tau_bp': 0.04, 'one_rdm': True, 'two_rdm': 'structure_factor'}})
    assert got['est'].energies == []
    close(numpy.array(got['est'].two_rdm), want['bp_two_rdm'])


@pytest.mark.parametrize("batched", [False, True])
def test_traj_hubbard_energies(golden, monkeypatch, batched):
    got = capture_bp(monkeypatch)
    run_hirsch(golden, monkeypatch, 'traj_hirsch_bp.npz', batched=batched,
               bp={'tau_bp': 0.04, 'one_rdm': True, 'evaluate_energy': True})
    want = golden('hubbard_bp_energy.npz')['bp_energies']
    assert len(got['est'].energies) == len(want)
    close(numpy.array(got['est'].energies), want)


# ---------------------------------------------------------------- 2. the kernel
def ueg_device(s):
    """A handle that holds the system only: afq_ueg_pair_sums needs neither trial nor walkers."""
    dev = AfqDevice(0)
    H1diag = numpy.array([numpy.diag(s.H1[0]).real, numpy.diag(s.H1[1]).real])
    dev.set_system_ueg(s.iA, s.iB, s.ikpq_i, s.ikpq_kpq, s.ipmq_i, s.ipmq_pmq, s.vqvec, s.vol, H1diag, s.ecore,
                       s.nup, s.ndown)
    return dev


def check_kernel(s, G):
    dev = ueg_device(s)
    try:
        E, two = dev.ueg_pair_sums(G)
        E2, two2 = dev.ueg_pair_sums(G)
        assert numpy.array_equal(E, E2) and numpy.array_equal(two, two2)           # same input, same bits
        for g, e, t in zip(G, E, two):
            we, wt = ueg_sf_ref.evaluate(s, g)
            close(t, wt)
            close(e, we)
    finally:
        dev.close()
    return E, two


@pytest.mark.parametrize("tag", ['u', 'p', 'c'])
@pytest.mark.parametrize("full", [False, True])
def test_kernel_against_the_reference(golden, tag, full):
    d = golden('ueg_sf_direct.npz')
    rs, nup, ndown, ecut = d[tag + '_sys']
    s = systems.UEG(float(rs), int(nup), int(ndown), float(ecut), full_lists=full)
    key = tag + ('f' if full else 't') + '_'
    dev = ueg_device(s)
    E, two = dev.ueg_pair_sums(d[tag + '_G'])
    dev.close()
    close(two, d[key + 'two_rdm'])
    close(E, d[key + 'E'])


def rand_G(n, M, seed):
    rng = numpy.random.RandomState(seed)
    return rng.normal(size=(n, 2, M, M)) + 1j * rng.normal(size=(n, 2, M, M))


# (rs, nup, ndown, ecut, full_lists, n): M = 19 (ecut 1), 33 (2), 57 (3), 93 (4), 123 (5)
@pytest.mark.parametrize("rs,nup,ndown,ecut,full,n", [
    (2.0, 7, 7, 4.0, False, 3),       # C2: M = 93, nq = 750, the reference's lists: spin block in LDS, a thread per q
    (2.0, 7, 7, 4.0, True, 3),        # C2 with the complete lists (up to 68 entries): spin block in LDS, a wave per q
    (2.0, 7, 7, 4.0, True, 256),      # 256 Green's functions
    (2.0, 7, 7, 4.0, True, 1),
    (2.0, 7, 7, 5.0, False, 3),       # M = 123: the block does not fit, the lists' 7 rows do
    (2.0, 7, 7, 5.0, True, 2),        # M = 123, every row listed: global gathers
    (2.0, 7, 3, 2.0, True, 3),        # polarised
    (2.0, 5, 0, 2.0, False, 3),       # ndown = 0
    (2.0, 5, 0, 2.0, True, 3),
    (2.0, 1, 1, 1.0, False, 3),       # one listed plane wave: most momentum transfers have empty lists
    (2.0, 19, 19, 3.0, False, 2),     # lists of 19: thread-per-q and wave-per-q in one launch
])
def test_kernel_dispatch_boundaries(rs, nup, ndown, ecut, full, n):
    s = systems.UEG(rs, nup, ndown, ecut, full_lists=full)
    check_kernel(s, rand_G(n, s.nbasis, 17 + n))


class ListSystem(object):
    """Synthetic index lists on M plane waves: rows anywhere in [0, M), lengths from 0 to M, for the sizes a real gas
    does not offer (the largest M the whole-block path takes is 99: 16 * 99 * 99 bytes of LDS; 100 is past it)."""

    def __init__(self, M, nq, nrows, seed):
        rng = numpy.random.RandomState(seed)
        self.nbasis, self.nup, self.ndown, self.ecore, self.vol = M, 2, 2, 0.0, 3.7
        rows = numpy.sort(rng.choice(M, size=nrows, replace=False))
        lens = rng.randint(0, nrows + 1, size=(2, nq))
        lens[:, :3] = 0                                    # empty lists
        lens[0, 3], lens[1, 3] = nrows, 0                  # one side empty
        lens[:, 4] = nrows                                 # the longest
        lens[:, 5] = 8                                     # nk * np = 64: the last a thread takes
        lens[0, 6], lens[1, 6] = 5, 13                     # 65: the first a wave takes
        lens = numpy.minimum(lens, nrows)
        mk = lambda k: [rng.choice(rows, size=lens[k, q], replace=False).astype(numpy.int64) for q in range(nq)]
        col = lambda ls: [rng.randint(0, M, size=len(x)).astype(numpy.int64) for x in ls]
        self.ikpq_i, self.ipmq_i = mk(0), mk(1)
        self.ikpq_kpq, self.ipmq_pmq = col(self.ikpq_i), col(self.ipmq_i)
        self.vqvec = rng.rand(nq) + 0.1
        self.qvecs = numpy.zeros((nq, 3))
        e = rng.rand(M)
        self.H1 = numpy.array([numpy.diag(e), numpy.diag(e)])
        import scipy.sparse
        self.iA = self.iB = scipy.sparse.csc_matrix((M * M, nq), dtype=numpy.complex128)


@pytest.mark.parametrize("M,nq,nrows,mode", [
    (99, 40, 99, 0),       # the largest spin block that goes to LDS whole
    (100, 40, 100, 2),     # that plus one, every row listed: global
    (100, 40, 98, 1),      # that plus one, 98 rows listed: those go to LDS
    (100, 40, 99, 2),      # 99 rows of pitch 101 are past the LDS budget
    (64, 70, 64, 0),       # even M: the pitch is M + 1
    (16, 1100, 9, 0),      # more momentum transfers than threads
])
def test_kernel_on_synthetic_lists(M, nq, nrows, mode):
    s = ListSystem(M, nq, nrows, seed=M + nrows)
    P = M | 1
    assert mode == (0 if 16 * M * P <= 156 * 1024 else 1 if 16 * nrows * P <= 156 * 1024 else 2)
    check_kernel(s, rand_G(3, M, 5))


def test_local_energy_fills_two_rdm(golden):
    d = golden('ueg_sf_direct.npz')
    s = systems.UEG(2.44, 7, 7, 2.0)
    t = trial_mod.hartree_fock_ueg(s)
    from pauxy_amd.context import get_context
    get_context(s, t)
    try:
        G = d['u_G'][0]
        two = numpy.zeros((2, 2, len(s.qvecs)), dtype=numpy.complex128)
        e = local_energy(s, G, two_rdm=two)
        close(two, d['ut_two_rdm'][0])
        close(numpy.array(e), d['ut_E'][0])
        # without two_rdm: the existing path, and the same energy when the rows beyond the trial's vanish
        Gm = numpy.zeros_like(G)
        Gm[:, :7] = G[:, :7]
        close(numpy.array(local_energy(s, Gm)), numpy.array(local_energy(s, Gm, two_rdm=two)))
    finally:
        release_context(s, t)


def test_refusals_on_other_systems():
    m = hubbard_model(4, 4, 3, 2)
    dev = make_device(m, 2)
    try:
        with pytest.raises(L.AfqError) as e:
            dev.ueg_pair_sums(numpy.zeros((1, 2, 16, 16), dtype=complex))
        assert e.value.code == -5                           # AFQ_EUNSUPPORTED
        with pytest.raises(L.AfqError) as e:
            dev.estimates_sf(True)
        assert e.value.code == -5
    finally:
        dev.close()
    from tests.test_gpu_bp_obs import build
    dev = make_device(build(12, 8, 2, 2)[0], 2)
    try:
        dev.bp_configure(2)
        with pytest.raises(L.AfqError) as e:
            dev.bp_observables(two_rdm='structure_factor')
        assert e.value.code == -5
    finally:
        dev.close()
    s = systems.UEG(2.0, 7, 7, 1.0)
    dev = ueg_device(s)
    try:
        with pytest.raises(L.AfqError) as e:
            dev.hubbard_energy_full_g(numpy.zeros((1, 2, s.nbasis, s.nbasis), dtype=complex))
        assert e.value.code == -5
    finally:
        dev.close()


# ---------------------------------------------------------------- 3. the window's sums on a device population
def ueg_model_of(s, dt=0.005):
    t = trial_mod.hartree_fock_ueg(s)
    BH1, mf = setup.ueg_propagator_arrays(s, t, dt)
    H1diag = numpy.array([numpy.diag(s.H1[0]).real, numpy.diag(s.H1[1]).real])
    return ref.RefModel('ueg', s.nbasis, s.nup, s.ndown, t.psi, BH1, mf, dt, iA=s.iA, iB=s.iB, H1diag=H1diag,
                        vqvec=s.vqvec, vol=s.vol, ikpq_i=s.ikpq_i, ikpq_kpq=s.ikpq_kpq, ipmq_i=s.ipmq_i,
                        ipmq_pmq=s.ipmq_pmq, ecore=s.ecore)


def run_window(s, nw, restore=None, zero=(), nbp=3, energy=True, seed=3):
    model = ueg_model_of(s)
    M, ne, K = s.nbasis, s.nup + s.ndown, 2 * len(s.qvecs)
    rng = numpy.random.RandomState(seed)
    dev = make_device(model, nw)
    try:
        dev.set(L.F_PHI, numpy.array([model.psi + 0.1 * (rng.rand(M, ne) + 1j * rng.rand(M, ne)) for _ in range(nw)]))
        dev.set(L.F_OT, dev.calc_overlap())
        dev.bp_configure(nbp)
        for step in range(nbp):
            dev.propagate(rng.normal(size=(nw, K)), 0.2)
        dev.bp_observables(two_rdm='structure_factor')
        w0 = dev.get(L.F_WEIGHT).copy()
        w0[list(zero)] = 0.0
        Gs, wts = [], []
        for i in range(nw):                       # every walker's G_bp and weight, as test_gpu_bp_obs.run_case does
            one = numpy.zeros(nw)
            one[i] = 1.0
            dev.set(L.F_WEIGHT, one)
            _, den, G = dev.bp_update(model.psi, 5, restore, reset=False)
            Gs.append(G / den)
            wts.append(den * w0[i])
        dev.set(L.F_WEIGHT, w0)
        E, den, G, extra = dev.bp_update(model.psi, 5, restore, energy, reset=False, two_rdm=True)
        wantE, want2 = ueg_sf_ref.window(s, Gs, wts)
        close(den, numpy.sum(wts), 1e-10)
        close(extra['two_rdm'], want2)
        close(E, wantE if energy else numpy.zeros(3))
        # 6. the same window from the same state again: the same bits
        E2, den2, G2, extra2 = dev.bp_update(model.psi, 5, restore, energy, reset=False, two_rdm=True)
        assert numpy.array_equal(extra2['two_rdm'], extra['two_rdm']) and numpy.array_equal(E2, E)
        assert numpy.array_equal(G2, G) and den2 == den
        # without the options: afq_bp_update as before, bitwise the same G_bp sums
        a = dev.bp_update(model.psi, 5, restore, reset=False)
        assert numpy.array_equal(a[2], G) and a[1] == den and not numpy.any(a[0])
    finally:
        dev.close()


@pytest.mark.parametrize("nup,ndown,ecut,full,nw,restore,zero,energy", [
    (7, 7, 2.0, False, 6, None, (), True),
    (7, 7, 2.0, True, 6, None, (), True),            # the complete sums
    (7, 7, 2.0, True, 5, 'partial', (), True),       # complex weights
    (7, 7, 2.0, True, 5, 'full', (1, 3), True),      # walkers of weight zero
    (7, 3, 2.0, True, 4, None, (), False),           # polarised; the structure factor without the energies
    (7, 7, 4.0, True, 3, None, (), True),            # C2's plane waves
])
def test_window_against_restatement(nup, ndown, ecut, full, nw, restore, zero, energy):
    run_window(systems.UEG(2.0, nup, ndown, ecut, full_lists=full), nw, restore, zero, energy=energy)


def test_two_path_lengths_through_the_driver(golden, monkeypatch):
    """nsplit = 2 with the complete lists: both path lengths give a window, slices and groups in place."""
    d = dict(golden('traj_bp_ueg.npz'))
    s = systems.UEG(float(d['sys_rs']), 7, 7, float(d['sys_ecut']), full_lists=True)
    t = trial_mod.hartree_fock_ueg(s)
    got = capture_bp(monkeypatch)
    bp = {'tau_bp': 0.04, 'one_rdm': True, 'evaluate_energy': True, 'two_rdm': 'structure_factor', 'nsplit': 2}
    # the lists do not enter the walk (mixed Green's functions of the Hartree-Fock trial): replay checks it as usual
    replay(d, s, t, {}, monkeypatch, est_extra={'back_propagated': bp}, batched=True)
    est = got['est']
    sp = numpy.array(est.split_of)
    assert set(sp) == {2, 4} and len(est.two_rdm) == len(sp) == len(est.energies)
    close(numpy.array(est.one_rdm)[sp == 4], d['bp_one_rdm'])
    vq = s.vqvec / (2.0 * s.vol)
    for e, two, den in zip(est.energies, est.two_rdm, est.denominator):
        close(numpy.dot(vq, two.sum(axis=(0, 1))) / den, e[2])           # E2b is the structure factor folded with v(q)


# ---------------------------------------------------------------- 4. Hubbard
def hubbard_model(nx, ny, na, nb, U=4.0, dt=0.01):
    s = systems.Hubbard(nx, ny, na, nb, U)
    M = s.nbasis
    rng = numpy.random.RandomState(2)
    psi = numpy.linalg.qr(rng.normal(size=(M, M)))[0][:, :na + nb].astype(complex)
    import scipy.linalg
    BH1 = numpy.array([scipy.linalg.expm(-0.5 * dt * s.h1e_mod[0]), scipy.linalg.expm(-0.5 * dt * s.h1e_mod[1])])
    return ref.RefModel('hubbard', M, na, nb, psi, BH1.astype(complex), numpy.zeros(M, dtype=complex), dt, U=U,
                        H1=s.T.astype(complex))


@pytest.mark.parametrize("nx,n", [(4, 3), (16, 2)])
def test_hubbard_full_g_energy(nx, n):
    m = hubbard_model(nx, nx, 3, 2)
    dev = make_device(m, 1)
    try:
        G = rand_G(n, nx * nx, 9)
        E = dev.hubbard_energy_full_g(G)
        assert numpy.array_equal(E, dev.hubbard_energy_full_g(G))
        for g, e in zip(G, E):
            close(e, ueg_sf_ref.hubbard_energy(m.H1, m.U, g))
    finally:
        dev.close()


# ---------------------------------------------------------------- 5. mixed estimator
def run_mixed(freq, batched, monkeypatch):
    s = systems.UEG(2.0, 7, 7, 1.0)
    t = trial_mod.hartree_fock_ueg(s)
    nsteps, nblocks, nw = 10, 2, 6
    options = {'qmc': {'timestep': 0.01, 'num_steps': nsteps, 'blocks': nblocks, 'stabilise_freq': 5,
                       'pop_control_freq': 5, 'num_walkers': nw, 'rng_seed': 7},
               'propagator': {'device_rng': False},
               'estimators': {'mixed': {'energy_eval_freq': freq, 'verbose': False, 'two_rdm': 'structure_factor'}}}
    numpy.random.seed(7)
    afqmc = AFQMC(options=options, system=s, trial=t)
    events, marks = [], {0: 0}
    upd = AfqDevice.estimates_update

    def update(self, eval_energy):
        upd(self, eval_energy)
        if eval_energy:
            events.append((self.get(L.F_WEIGHT).copy(), self.get(L.F_G).copy()))
    monkeypatch.setattr(AfqDevice, 'estimates_update', update)

    def on_step(step, psi):
        marks[step] = len(events)
    if batched:
        afqmc.run_batched(on_step=on_step, fetch_popcontrol=True)
    else:
        afqmc.run(verbose=False, on_step=on_step)
    mixed = afqmc.estimators.estimators['mixed']
    blocks = numpy.array(mixed.blocks)
    assert len(mixed.two_rdm) == nblocks == len(blocks)
    vq = s.vqvec / (2.0 * s.vol)
    for b in range(nblocks):
        ev = events[marks[b * nsteps]:marks[(b + 1) * nsteps]]
        assert len(ev) == nsteps // freq + (1 if b == 0 else 0)
        num = sum(w * ueg_sf_ref.evaluate(s, g)[1].real for wts, Gs in ev for w, g in zip(wts, Gs))
        den = sum(wts.sum() for wts, Gs in ev)
        two = mixed.two_rdm[b]
        assert two.shape == (2, 2, len(s.qvecs)) and two.dtype == numpy.float64
        close(two, num / den)
        close(numpy.dot(vq, two.sum(axis=(0, 1))), blocks[b, 7].real)       # the block's E2Body column
    afqmc.finalise()
    release_context(s, t)


@pytest.mark.parametrize("freq", [1, 5])
@pytest.mark.parametrize("batched", [False, True])
def test_mixed_structure_factor(freq, batched, monkeypatch):
    run_mixed(freq, batched, monkeypatch)
