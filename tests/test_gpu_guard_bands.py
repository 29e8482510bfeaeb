"""Every kernel family under the guard mode of the handle's device memory (AFQ_DEBUG_GUARD, pauxy_amd/csrc/dev_guard.h).

The rest of the suite compares results, and results cannot show a store that lands outside its buffer -- every block is
allocated to the element, and a missed predicate writes into the allocator's rounding space or a neighbouring block -- nor a
read of memory nobody wrote, which a fresh process mostly gets as zero pages.  Here each row runs one EXISTING case runner of
the suite (imported, not copied: it creates, uses, value-checks and closes its own device) under
  mode 1: a 64 KiB band of a NaN word in front of and behind every device block of the handle, compared with the pattern when
          the block is freed: a row fails if afq_debug_guard_report has anything to say;
  mode 2: the bands, and every block of double / complex elements filled with a second NaN word before it is handed out
          (index and counter blocks with zeros): the runner's own value checks are the detector -- a NaN that reached a
          result fails them exactly as they stand -- and the digest rows reproduce their recorded SHA-256 literals with ==.
The shapes are the smallest of the suite at which the tile edges are ragged, so the reference side is known to pass.

What neither mode sees: a store further than one band from its block; stray accesses that land inside another live block;
reads that an fmax-style select swallows (only the digest rows catch those).  profiles/guard_bands.md has the kernel names
each family launched, the findings and the mutations this module was tried against."""
import numpy
import pytest

from pauxy_amd import _lib as L

pytestmark = pytest.mark.gpu
BAND = 65536
MODES = [1, 2]


modes = pytest.mark.parametrize("mode", MODES, ids=lambda m: "mode%d" % m)


def guard_report():
    import ctypes
    buf = ctypes.create_string_buffer(16384)
    n = int(L.load().afq_debug_guard_report(buf, 16384))
    return n, buf.value.decode(errors='replace')


def under_guard(monkeypatch, mode, run):
    """run() with every handle it creates in the guard mode; nothing may have touched a band."""
    monkeypatch.setenv("AFQ_DEBUG_GUARD", str(mode))
    monkeypatch.setenv("AFQ_DEBUG_GUARD_BYTES", str(BAND))
    L.load().afq_debug_guard_reset()
    try:
        out = run()
    except BaseException as failed:
        n, text = guard_report()
        L.load().afq_debug_guard_reset()
        if n:                                   # say so beside the runner's own failure
            raise AssertionError("the runner failed, and bands were written:\n" + text) from failed
        raise
    n, text = guard_report()
    L.load().afq_debug_guard_reset()
    assert n == 0, text
    return out


def rows(table):
    return [pytest.param(fn, id=name) for name, fn in table]


# ------------------------------------------------------------------------------------------------ the facility on the device
@modes
def test_the_mode_is_on_and_the_handle_sees_it(monkeypatch, mode):
    """A plane-wave handle allocates walker.G with the walkers and nothing writes it before the first Green's function: under
    mode 2 it reads back as the poison word, under mode 1 as whatever the allocation held.  afq_debug_guard_check walks the
    live blocks and finds the bands intact; afq_thermal_device_allocations counts what it counts without the mode."""
    from tests.helpers import make_device
    from tests.test_gpu_sizes import ueg_model_of
    model = ueg_model_of(1.0, 1, 1, 1.0)

    def run():
        dev = make_device(model, 3)
        try:
            G = dev.get(L.F_G)
            dev.guard_check()
            return numpy.ascontiguousarray(G).view(numpy.uint32), dev.thermal_device_allocations(), dev.guard_report()
        finally:
            dev.close()

    words, allocated, (n, text) = under_guard(monkeypatch, mode, run)
    assert n == 0, text
    if mode == 2:
        assert numpy.all(words == 0x7ff8feed) and numpy.all(numpy.isnan(words.view(numpy.float64)))
    monkeypatch.delenv("AFQ_DEBUG_GUARD")
    dev = make_device(model, 3)
    try:
        assert dev.thermal_device_allocations() == allocated
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ generic systems
def generic(M, K, na, nb, nw, cplx, lform='real'):
    def run():
        from tests.test_gpu_shape_sweep import run_shape
        run_shape(M, K, na, nb, nw, cplx, lform)
    return "%d-%d-%d+%d-nw%d-%s-%s" % (M, K, na, nb, nw, "T" if cplx else "F", lform), run


GENERIC = [
    generic(37, 45, 7, 6, 70, False),                   # reortho_fused_kernel<4>
    generic(200, 12, 10, 9, 65, True),                  # reortho_fused_kernel<8>
    generic(105, 9, 26, 25, 64, True, 'hermitian'),     # reortho_fused_kernel<13>
    generic(104, 9, 32, 31, 64, False, 'general'),      # reortho_fused_kernel<16>
    generic(64, 20, 40, 37, 70, False),                 # LDS Gauss-Jordan, GEMM-engine QR
    generic(130, 16, 20, 20, 70, False),                # M > 128
    generic(18, 5, 4, 3, 33, True, 'hermitian'),
    generic(19, 4, 3, 3, 32, False, 'general'),
]
# the cplx flag of each shape is the one tests.test_gpu_shape_sweep runs it with
DEGENERATE = [generic(2, 1, 1, 1, 1, False), generic(6, 3, 2, 0, 7, False), generic(5, 3, 1, 1, 257, True),
              generic(16, 5, 16, 15, 64, False), generic(17, 1, 8, 8, 63, False), generic(33, 4, 1, 0, 64, True)]


@pytest.mark.parametrize("run", rows(GENERIC))
@modes
def test_generic_gemms_fused_propagator_greens_and_qr(monkeypatch, mode, run):
    under_guard(monkeypatch, mode, run)


@pytest.mark.parametrize("run", rows(DEGENERATE))
@modes
def test_degenerate_shapes(monkeypatch, mode, run):
    under_guard(monkeypatch, mode, run)


def blocked(which, M, na, nb):
    def run():
        from tests import test_gpu_sizes as S
        {'gauss-jordan': S.test_blocked_gauss_jordan_hands_badly_placed_pivots_to_the_step_by_step_kernel,
         'cholesky': S.test_blocked_cholesky_reortho_every_tile_count}[which](M, na, nb)
    return "%s-%d-%d+%d" % (which, M, na, nb), run


@pytest.mark.parametrize("run", rows([blocked(w, *s) for w in ('gauss-jordan', 'cholesky')
                                      for s in ((140, 64, 40), (150, 128, 97), (130, 113, 17))]))
@modes
def test_blocked_gauss_jordan_and_cholesky(monkeypatch, mode, run):
    """The bodies of the two k_bigdet.hip tests of tests.test_gpu_sizes at the three shapes asked for.  The suite runs the
    Cholesky body at (130, 113, 17) but not the Gauss-Jordan body, whose constructions are made for spins of more than 32
    orbitals: applied to the 17 beta orbitals, the leading tile scaled by 1e-10 left a 17 x 17 overlap matrix of condition
    number 9.0e10 (1.7e2 for the 113 alpha orbitals), and the device -- fallback pass included, with and without the mode,
    no band touched -- differed from the oracle's LAPACK inverse by 1.45e-6 in the overlap and 2.97e-6 in the beta Ghalf,
    as any two fp64 inverses may there (condition x 2.2e-16 = 2e-5), against the body's 1e-9 and 1e-8.  The body now leaves
    a spin of 32 orbitals or fewer its ordinary walkers; its own shapes have no such spin and run what they ran."""
    under_guard(monkeypatch, mode, run)


# ------------------------------------------------------------------------------------------------ resident propagator
def recorded_step(M, n, nw):
    """The fused step with everything on (product through three multiplications, tail in the launch, early overlap,
    hand-over): the recorded literals of tests.test_gpu_step_plan, traces, counters and SHA-256, with ==."""
    def run():
        from tests import test_gpu_step_plan as P
        name = 'resident %d, %d' % (M, n) + (': fusion 2 scope 1 overlap 1 hand-over 1' if nw == 33 else '')
        P.test_a_launch_is_what_it_was_before_the_plan(name)
    return "recorded-%d-%d-nw%d" % (M, n, nw), run


def repeated_step(M, n, nw):
    """Shapes tests.test_gpu_step_plan has no literals for: the same three steps unguarded first, then under the mode; traces,
    counters, issued flops and the SHA-256 of phi, weights and overlaps must be equal."""
    def run():
        from tests import test_gpu_step_plan as P
        return P.measure(P.case('guard %d, %d' % (M, n), M, n, n, nw=nw))
    return "repeated-%d-%d-nw%d" % (M, n, nw), run


@pytest.mark.parametrize("run", rows([recorded_step(100, 25, 33), recorded_step(97, 17, 33)]))
@modes
def test_resident_step_reproduces_its_recorded_digests(monkeypatch, mode, run):
    under_guard(monkeypatch, mode, run)


@pytest.mark.parametrize("run", rows([repeated_step(98, 28, 4), repeated_step(40, 13, 4)]))
@modes
def test_resident_step_has_the_bits_it_has_without_the_mode(monkeypatch, mode, run):
    monkeypatch.delenv("AFQ_DEBUG_GUARD", raising=False)
    plain = run()
    guarded = under_guard(monkeypatch, mode, run)
    assert any('prop_fused_kernel' in name for name, _n in plain[0][0]), plain[0][0]
    assert guarded == plain


# ------------------------------------------------------------------------------------------------ multi-determinant trials
def nomsd(*row):
    def run():
        from tests.test_gpu_shape_sweep import test_distinct_complex_determinants_on_boundary_shapes as body
        body(*row, 'real')
    return "-".join(str(x) for x in row[:6]) + ("-zero-coeff" if row[6] else ""), run


def dead_determinant():
    from tests.test_gpu_msd import test_numerically_dead_determinant_is_skipped_like_the_reference as body
    body(1, 3, 3, 12)


def dead_walkers_from_the_start():
    """Two of five walkers have weight zero before the handle computes anything: the step must not count a determinant
    overlap of theirs that nothing wrote as a numerical failure (afq_counters_ext [6]), whatever the allocation held."""
    from oracle import afqmc_ref as ref
    from tests.conftest import load_golden
    from tests.helpers import make_device, msd_model
    from tests.test_gpu_msd import close
    d = load_golden('msd_ops.npz')
    m = msd_model(d, 'N_')
    nw, dead = 5, (1, 3)
    rng = numpy.random.RandomState(9)
    phi0 = d['N_phi0'][None] + 0.05 * (rng.rand(nw, m.M, m.na + m.nb) + 1j * rng.rand(nw, m.M, m.na + m.nb))
    w0 = numpy.ones(nw)
    w0[list(dead)] = 0.0
    xi = rng.normal(size=(nw, m.nfields))
    dev = make_device(m, nw, hybrid=True)
    try:
        dev.set(L.F_PHI, phi0)
        dev.set(L.F_WEIGHT, w0)
        dev.set(L.F_OT, numpy.array([m.greens(p)[0] for p in phi0]))
        dev.counters(reset=True, n=10)
        dev.propagate(xi, 0.1)
        phi, wt = dev.get(L.F_PHI), dev.get(L.F_WEIGHT)
        assert int(dev.counters(n=10)[6]) == 0
        assert numpy.all(numpy.isfinite(dev.det_weights()[[i for i in range(nw) if i not in dead]]))
        for i in range(nw):
            if i in dead:
                assert numpy.array_equal(phi[i], phi0[i]) and wt[i] == 0.0
                continue
            w = ref.new_walker(m, phi0[i])
            ref.propagate_walker_phaseless(m, w, xi[i], 0.1, hybrid=True)
            close(phi[i], w['phi'], 1e-9)
            close(wt[i], w['weight'], 1e-9)
    finally:
        dev.close()


@pytest.mark.parametrize("run", rows([nomsd(24, 10, 5, 4, 3, 33, True), nomsd(65, 10, 20, 19, 3, 40, True),
                                      ("dead-determinant", dead_determinant),
                                      ("dead-walkers-from-the-start", dead_walkers_from_the_start)]))
@modes
def test_multi_determinant_trials(monkeypatch, mode, run):
    under_guard(monkeypatch, mode, run)


# ------------------------------------------------------------------------------------------------ Hubbard
def hubbard_continuous(nx, ny, na, nb, nw):
    def run():
        from tests.test_gpu_shape_sweep import test_hubbard_continuous_on_boundary_shapes as body
        body(nx, ny, na, nb, nw, False)
    return "continuous-%dx%d-%d+%d-nw%d" % (nx, ny, na, nb, nw), run


def hirsch(nx, ny, na, nb, nw):
    def run():
        from tests.test_gpu_fullsize import run_hirsch_lattice
        run_hirsch_lattice(nx, ny, na, nb, False, nw)
    return "hirsch-%dx%d-%d+%d-nw%d" % (nx, ny, na, nb, nw), run


@pytest.mark.parametrize("run", rows([hubbard_continuous(3, 3, 5, 4, 33), hubbard_continuous(7, 7, 24, 23, 66),
                                      hubbard_continuous(12, 11, 66, 66, 9), hirsch(3, 3, 5, 4, 7), hirsch(9, 9, 40, 33, 4),
                                      hirsch(12, 12, 72, 70, 3)]))
@modes
def test_hubbard_continuous_and_hirsch(monkeypatch, mode, run):
    under_guard(monkeypatch, mode, run)


# ------------------------------------------------------------------------------------------------ plane waves
def ueg(rs, nup, ndown, ecut, nw):
    def run():
        from tests.test_gpu_fullsize import run_fullsize
        from tests.test_gpu_sizes import ueg_model_of
        run_fullsize(ueg_model_of(rs, nup, ndown, ecut), nw, sorted({0, 2, nw // 2, nw - 1}))
    return "%g-%d+%d-ecut%g-nw%d" % (rs, nup, ndown, ecut, nw), run


def ueg_step(rs, nup, ndown, ecut, rotated):
    def run():
        from tests import test_gpu_sizes as S
        S.test_planewave_step_shapes(rs, nup, ndown, ecut, S.rotated_trial if rotated else None)
    return "step-%g-%d+%d-ecut%g%s" % (rs, nup, ndown, ecut, "-rotated-trial" if rotated else ""), run


@pytest.mark.parametrize("run", rows([ueg(1.0, 1, 1, 1.0, 5), ueg_step(1.0, 7, 5, 2.5, False), ueg(2.0, 7, 7, 4.0, 5),
                                      ueg(2.0, 19, 19, 3.0, 8), ueg_step(2.0, 7, 7, 2.5, True)]))
@modes
def test_plane_wave_steps(monkeypatch, mode, run):
    under_guard(monkeypatch, mode, run)


# ------------------------------------------------------------------------------------------------ windows and estimators
def bp_obs_dispatch():
    from tests.test_gpu_bp_obs import run_case
    run_case(17, 20, 3, 4, 4, True, True, restore='full', own_L=False, nL=13)          # general complex L, odd nL


def bp_obs_chunks():
    from tests.test_gpu_bp_obs import run_case
    run_case(21, 14, 4, 3, 5, False, True, restore='partial', sym=False, chunks=(4, 5))  # L^T panels: 3 + 1, 2 + 1 chunks


def itcf(table, prefix):
    def run():
        from tests import test_gpu_itcf_shapes as I
        (case, kw), = [r for r in getattr(I, table) if r[0].startswith(prefix)]
        I.run_generic(case, **kw)
    return "itcf-" + prefix.replace(' ', '-').replace('=', ''), run


def itcf_hirsch():
    from tests import test_gpu_itcf_shapes as I
    (case, kw), = [r for r in I.HIRSCH if r[0] == "hirsch 3x3 5+4"]
    I.test_hirsch_lattices_and_the_charge_decomposition(case, kw)


def bp_msd():
    from tests import test_gpu_bp_msd as B
    (case, kw), = [r for r in B.SHAPES if r[0].startswith("M=24 5+6 ndet=2 na<nb, two dead")]
    B.run(case, **kw)


def corr():
    from tests import test_gpu_corr as C
    C.test_kernel_on_every_tile_boundary(C.T + 1, 3, 'hubbard')
    C.test_window_hubbard(5, True)


def pair():
    from tests import test_gpu_pair as P
    P.test_kernel_on_every_tile_boundary(P.T + 1, 3, 5)
    P.test_window_hubbard(5, True)


def ueg_sf():
    from tests.test_gpu_ueg_sf import test_window_against_restatement as body
    body(7, 3, 2.0, True, 4, None, (), False)           # polarised: ragged spin blocks


@pytest.mark.parametrize("run", rows([("bp-obs-dispatch", bp_obs_dispatch), ("bp-obs-chunks", bp_obs_chunks),
                                      itcf('BACKWARD', "M=33 4+0"), itcf('GEMM_EDGES', "M=33 5+4"), ("itcf-hirsch-3x3", itcf_hirsch),
                                      ("bp-msd", bp_msd), ("corr", corr), ("pair", pair), ("ueg-sf", ueg_sf)]))
@modes
def test_windows_and_estimators(monkeypatch, mode, run):
    under_guard(monkeypatch, mode, run)


# ------------------------------------------------------------------------------------------------ walker moves, one rank
def walker_move(name):
    def run():
        from tests import test_gpu_walker_state as W
        from tests.conftest import load_golden
        from tests.helpers import generic_model
        getattr(W, name)(generic_model(load_golden('generic_ops.npz'), 'A_'))
    return name[5:].replace('_', '-'), run


def comb_with_clones():
    """A comb of eight walkers of weights exp(N(0, 1)) -- clones and kills -- behind a step that left a cached Green's
    function, with and without a one-rank window communicator (whose windows are not guarded; the handle's blocks are)."""
    from tests import test_gpu_comm as C
    from tests.conftest import load_golden
    cache = {}
    C.test_ipc_communicator_of_one_rank(lambda name: cache.setdefault(name, load_golden(name)))


@pytest.mark.parametrize("run", rows([walker_move('test_one_rank_comb'), walker_move('test_one_rank_pair_branch'),
                                      walker_move('test_copy_walker'), walker_move('test_pack_and_unpack_into_another_index'),
                                      ("comb-with-clones", comb_with_clones)]))
@modes
def test_population_control_and_walker_moves(monkeypatch, mode, run):
    under_guard(monkeypatch, mode, run)


# ------------------------------------------------------------------------------------------------ thermal walkers
def thermal_real_resident():
    from tests import test_gpu_thermal as T
    from tests.thermal_cases import Case
    T.greens_case(Case(3, 3, 4.0, 0.05), 4, 5, [0])
    T.test_full_path_against_the_extended_restatement(3, 3, 10, 5, 5, 5)


def thermal_delayed():
    from tests import test_gpu_thermal_delayed as T
    T.test_wide_real_greens_from_an_uploaded_stack(5, 13, 4)
    T.test_full_path_against_the_extended_restatement(5, 13, 10, 5, 5, 2)


def thermal_complex(M, streamed):
    def run():
        if streamed:
            from tests.test_gpu_thermal_ueg_streamed import greens_case
        else:
            from tests.test_gpu_thermal_ueg import greens_case
        greens_case(M, 2, 5, [0], nw=3)
    return "complex-%s-%d" % ("streamed" if streamed else "resident", M), run


def thermal_wide():
    from tests import test_gpu_thermal_wide as T
    T.greens_case(19, 2, 2, [0])
    T.path_against_restatement(T.chain(19), 2, 2, 4, 49, "M=19")


def thermal_hubbard_continuous():
    from tests import test_gpu_thermal_hubbard_cont as T
    T.path_against_restatement(T.C.Chain(9), 2, 3, 0, 4, 23, "M=9")


def thermal_sweep():
    from tests.test_gpu_thermal_obs import test_chunked_sweep_gives_the_same_bits_and_the_launches_are_pinned as body
    body('real', 9)


def thermal_digest(key):
    def run():
        from tests.test_gpu_thermal_route_bits import test_wide_and_delayed_routes_keep_their_bits as body
        body(key)
    return "digest-" + key.replace(' ', '-'), run


@pytest.mark.parametrize("run", rows([("real-resident-3x3", thermal_real_resident), ("delayed-5x13", thermal_delayed),
                                      thermal_complex(7, False), thermal_complex(19, False), thermal_complex(7, True),
                                      thermal_complex(19, True), ("wide-19", thermal_wide),
                                      ("hubbard-continuous-9", thermal_hubbard_continuous), ("average-gf-two-chunks", thermal_sweep),
                                      thermal_digest('delayed 5x13'), thermal_digest('complex wide Green 19')]))
@modes
def test_thermal_walkers(monkeypatch, mode, run):
    under_guard(monkeypatch, mode, run)
