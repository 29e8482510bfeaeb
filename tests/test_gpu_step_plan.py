"""What a fused-propagator launch IS -- the instantiation, the tile deal, the tail, the early overlap, the step hand-over --
is decided by one plan (pauxy_amd/csrc/step_plan.h).  This file holds every instantiation, and the decision boundaries
between them, to what the library launched, counted and computed BEFORE the plan existed: the literals below were recorded
with the build of the parent commit on an MI355X and are compared with ==.  The device code did not change and the inputs
are fixed, so equality is the test.

Cases: K = 8, order 2, three steps (announced, unannounced, announced) on the device's own Philox fields.  Four walkers, of
which walker 3 has weight zero and, where na == nb (closed walkers exist), walker 1 is open-shell.  The step's Green's
function rides on the propagator only where the force bias contracts the spin sum -- more than 32 walkers -- so the
resident class is ALSO run with 33 walkers (same open and dead walker): only there do the two tail instantiations launch.
Every (step fusion, scope, tail overlap, hand-over) setting is crossed there; (overlap, hand-over) = (0, 1) is (0, 0) by
construction (the hand-over exists under the overlap alone), as in tests.test_gpu_taylor_deal.SWITCHES.

Behind each step: the launch-trace names in order with their counts, afq_counters_ext [3] and [9], the propagator's issued
flops per walker (open, closed) and per launch, and a SHA-256 over the bytes of phi, the weights and the overlaps of the
propagated walkers (ovlp_new, read as F_OT behind the step).  tests/test_step_plan_cpu.py holds the plan itself, computed on
the host, to the same literals."""
import functools
import hashlib

import numpy
import pytest

from oracle import afqmc_ref as ref
from pauxy_amd import _lib as L
from tests.helpers import make_device
from tests.test_gpu_sizes import build
from tests.test_gpu_step_fusion import ESHIFT, SEED

K, ORDER = 8, 2
OPEN, DEAD = 1, 3
KINDS = ('announced', 'unannounced', 'announced')
RESIDENT = [(97, 17), (100, 25), (104, 32)]
SWITCHES = [(1, 1), (1, 0), (0, 0)]          # (tail overlap, step hand-over)


def case(name, M, na, nb, nw=4, onebody='same-real', closed_form=None, fusion=None, scope=None, overlap=None, handover=None):
    return dict(name=name, M=M, na=na, nb=nb, nw=nw, onebody=onebody, closed_form=closed_form, fusion=fusion, scope=scope,
                overlap=overlap, handover=handover)


CASES = [
    case('narrow generic', 20, 5, 3),
    case('narrow full', 90, 8, 8),
    case('wide generic', 40, 20, 18),
    case('wide full 5', 72, 17, 17),
    case('wide full 5, no closed_try', 72, 18, 17),
    case('wide full 6', 88, 17, 17),
    case('wide full 7, open', 104, 20, 18),
    case('contiguous, hyb', 100, 26, 24),
    case('contiguous, symcols, closed form 1', 100, 25, 25, closed_form=1),
    # edges of the resident class, below and above the population at which the tail rides
    case('M = 96', 96, 25, 25), case('M = 105', 105, 25, 25), case('n = 16', 100, 16, 16), case('n = 33', 100, 33, 33),
    case('M = 96, 33 walkers', 96, 25, 25, nw=33), case('M = 105, 33 walkers', 105, 25, 25, nw=33),
    case('n = 16, 33 walkers', 100, 16, 16, nw=33), case('n = 33, 33 walkers', 100, 33, 33, nw=33),
    # one complex one-body matrix for both spins (3 multiplications, no resident body); two real ones (no closed_try)
    case('complex BH1', 100, 25, 25, onebody='same-complex'), case('spin-dependent BH1', 100, 25, 25, onebody='spin-real'),
    case('complex BH1, 33 walkers', 100, 25, 25, nw=33, onebody='same-complex'),
    case('spin-dependent BH1, 33 walkers', 100, 25, 25, nw=33, onebody='spin-real'),
]
CASES += [case('resident %d, %d' % (M, n), M, n, n) for M, n in RESIDENT]
CASES += [case('resident %d, %d: fusion %d scope %d overlap %d hand-over %d' % (M, n, f, s, on, ho), M, n, n, nw=33,
               fusion=f, scope=s, overlap=on, handover=ho)
          for M, n in RESIDENT for f in (0, 1, 2) for s in (0, 1) for on, ho in SWITCHES]
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def population(M, na, nb, nw, onebody):
    model, rng = build(M, K, na, nb, False, seed=31)
    model.exp_order = ORDER
    if onebody == 'same-complex':
        pert = 1e-3 * (rng.rand(M, M) + 1j * rng.rand(M, M))
        model.BH1 = model.BH1 + numpy.array([pert, pert])
    elif onebody == 'spin-real':
        model.BH1 = model.BH1 + 1e-3 * rng.rand(2, M, M)
    if na == nb:
        half = model.psi[None, :, :na] + 0.1 * (rng.rand(nw, M, na) + 1j * rng.rand(nw, M, na))
        phis = numpy.concatenate([half, half], axis=2)
        phis[OPEN, :, na:] += 0.05 * (rng.rand(M, na) + 1j * rng.rand(M, na))
    else:
        phis = model.psi[None] + 0.1 * (rng.rand(nw, M, na + nb) + 1j * rng.rand(nw, M, na + nb))
    w0 = numpy.ones(nw)
    w0[DEAD] = 0.0
    ot = numpy.array([ref.calc_overlap(p, model.psi, na, nb) for p in phis])
    for a in (phis, w0, ot):
        a.setflags(write=False)
    return dict(model=model, phis=phis, w0=w0, ot=ot)


def measure(c):
    """The three steps of one case -> per step (trace, counter [3], counter [9], (open, closed), launch total, sha256)."""
    pop = population(c['M'], c['na'], c['nb'], c['nw'], c['onebody'])
    dev = make_device(pop['model'], c['nw'])
    try:
        for value, setter in ((c['closed_form'], dev.set_propagator_closed_form), (c['fusion'], dev.set_step_fusion),
                              (c['scope'], dev.set_step_fusion_scope), (c['overlap'], dev.set_step_tail_overlap),
                              (c['handover'], dev.set_step_handover)):
            if value is not None:
                setter(value)
        dev.rng_seed(*SEED)
        dev.set(L.F_PHI, pop['phis'])
        dev.set(L.F_WEIGHT, pop['w0'])
        dev.set(L.F_OT, pop['ot'])
        dev.counters(reset=True, n=10)
        out = []
        for how in KINDS:
            dev.launch_trace(True)
            if how == 'announced':
                dev.estimates_fuse_next()
            dev.propagate(None, ESHIFT)
            trace = tuple((name, n) for name, (n, _ms) in dev.launch_trace_get().items())
            dev.launch_trace(False)
            counted = dev.counters(n=10)
            sha = hashlib.sha256()
            for f in (L.F_PHI, L.F_WEIGHT, L.F_OT):
                sha.update(numpy.ascontiguousarray(dev.get(f)).tobytes())
            out.append((trace, int(counted[3]), int(counted[9]), tuple(float(x) for x in dev.propagator_issued_flops()),
                        float(dev.kernel_issued_flops(L.K_PROPAGATOR)), sha.hexdigest()))
        return tuple(out)
    finally:
        dev.close()


# The distinct launch traces of a step, and per case and step (index into TRACES, [3], [9], (open, closed), total, sha256):
# recorded with the library of the parent commit (the build before the plan), by measure() above.
TRACES = (
    (('(greens_tiny_kernel<true>)', 2), ('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('(prop_fused_kernel<true, 0>)', 1)),
    (('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('(prop_fused_kernel<true, 0>)', 1), ('(greens_tiny_kernel<true>)', 1)),
    (('(greens_tiny_kernel<true>)', 2), ('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('(prop_fused_kernel<true, 6>)', 1)),
    (('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('(prop_fused_kernel<true, 6>)', 1), ('(greens_tiny_kernel<true>)', 1)),
    (('(greens_small_kernel<true, true>)', 2), ('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('(prop_fused_kernel<false, 0>)', 1)),
    (('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('(prop_fused_kernel<false, 0>)', 1), ('(greens_small_kernel<true, true>)', 1)),
    (('(greens_small_kernel<true, true>)', 2), ('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('(prop_fused_kernel<false, 5>)', 1)),
    (('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('(prop_fused_kernel<false, 5>)', 1), ('(greens_small_kernel<true, true>)', 1)),
    (('(greens_small_kernel<true, true>)', 2), ('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('(prop_fused_kernel<false, 6>)', 1)),
    (('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('(prop_fused_kernel<false, 6>)', 1), ('(greens_small_kernel<true, true>)', 1)),
    (('(greens_small_kernel<true, true>)', 2), ('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('(prop_fused_kernel<false, 7>)', 1)),
    (('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('(prop_fused_kernel<false, 7>)', 1), ('(greens_small_kernel<true, true>)', 1)),
    (('rng_normal_kernel', 1), ('(greens_small_kernel<true, true>)', 2), ('onebody_spin', 4), ('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('k_apply_exponential', 2)),
    (('rng_normal_kernel', 1), ('onebody_spin', 4), ('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('k_apply_exponential', 2), ('(greens_small_kernel<true, true>)', 1)),
    (('(greens_small_kernel<true, true>)', 2), ('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('(prop_fused_kernel<true, 0>)', 1)),
    (('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('(prop_fused_kernel<true, 0>)', 1), ('(greens_small_kernel<true, true>)', 1)),
    (('rng_normal_kernel', 1), ('(greens_small_kernel<true, false>)', 2), ('onebody_spin', 4), ('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('k_apply_exponential', 2)),
    (('rng_normal_kernel', 1), ('onebody_spin', 4), ('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('k_apply_exponential', 2), ('(greens_small_kernel<true, false>)', 1)),
    (('(greens_small_kernel<true, true>)', 1), ('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('(prop_fused_kernel<false, 7, true, false>)', 1)),
    (('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('(prop_fused_kernel<false, 7, true, false>)', 1)),
    (('(greens_small_kernel<true, true>)', 1), ('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('(prop_fused_kernel<false, 7, true, true>)', 1)),
    (('force_bias_generic_impl', 1), ('fields_kernel<true>', 1), ('k_vhs_generic', 1), ('(prop_fused_kernel<false, 7, true, true>)', 1)),
)
BEFORE = {
    'narrow generic': (
        (0, 0, 0, (491520.0, 344064.0), 1966080.0, '7b2f94793367eeea051af87856313594b263211e01579d8ddb93b444cc515bc3'),
        (1, 0, 0, (491520.0, 344064.0), 1966080.0, '9f741e617090db4f46b7b23bf59951cfa92628496523aca5701bde34be838e52'),
        (1, 0, 0, (491520.0, 344064.0), 1966080.0, 'e5ce2a19c8dd840b8bc01b4f5c329ed952c273dfb6d97ac83c4504c0533ad1f5'),
    ),
    'narrow full': (
        (2, 2, 0, (5898240.0, 4128768.0), 23592960.0, '653efd449163debdc850fec64e648a971bb2edf59c052f0373aa610a0037dc6d'),
        (3, 4, 0, (5898240.0, 4128768.0), 23592960.0, 'de7cd04426e5c3c0312aacc158093b654827c47643cb11666a0ba86cc5351dc3'),
        (3, 6, 0, (5898240.0, 4128768.0), 23592960.0, 'a25bf87fd850dbb2af205b0b4eb65069f32d732dcf908b48b284c2129015ef78'),
    ),
    'wide generic': (
        (4, 0, 0, (2457600.0, 1720320.0), 9830400.0, 'c344f75549c6f51b9bc59fe9f2e2467e2b8b18fc1b67b820558fbe57e783c537'),
        (5, 0, 0, (2457600.0, 1720320.0), 9830400.0, 'e3f9b2bb8e2bd3cdd96c5550b035dfb865ed27654b57a674ca6db0050fcb2a01'),
        (5, 0, 0, (2457600.0, 1720320.0), 9830400.0, 'b2dae0a376332621f3080d3f5f02e626ede326b421126f4c2e9ffc2bd8de77c4'),
    ),
    'wide full 5': (
        (6, 2, 0, (7372800.0, 5160960.0), 29491200.0, '778b2d26cea1f00b5511f59e31313af2e569ba4a2f6b68f6c901e243508eaadb'),
        (7, 4, 0, (7372800.0, 5160960.0), 29491200.0, '784359833f9c67194ae7bf13539e5b557fe8ecc53a5aed12b7f58c96f025af8d'),
        (7, 6, 0, (7372800.0, 5160960.0), 29491200.0, 'd79a5739e5d0dfb7a1e01cdbe471e0de31286b9449c855e1b030ed815c8d894e'),
    ),
    'wide full 5, no closed_try': (
        (6, 0, 0, (7372800.0, 5160960.0), 29491200.0, 'beedb48cea883ce123b94a5ee7108b7c810a76a4c48910c120be32827c89340d'),
        (7, 0, 0, (7372800.0, 5160960.0), 29491200.0, '5b939678bc303395fd8568d18551ce24f6b175e81563a7d509f62a832eb8fccd'),
        (7, 0, 0, (7372800.0, 5160960.0), 29491200.0, '3eea14ea695f9d596ae1d64eb44b98a26ecf5a8fe2160b26dd928bd972b96007'),
    ),
    'wide full 6': (
        (8, 2, 0, (10813440.0, 7569408.0), 43253760.0, 'e60109b5ff07521f00430a20e69bc1765ce0fe6c45ca92d29bbf34dec777c96c'),
        (9, 4, 0, (10813440.0, 7569408.0), 43253760.0, 'a5edf1edd6dc1ffbec7751de510ceaf1a040638f7837337d44ec835a85782f4a'),
        (9, 6, 0, (10813440.0, 7569408.0), 43253760.0, '3532a0da504bb9521c35893c082ab067c67c5cad6e3b5b57db8bddfe4f773044'),
    ),
    'wide full 7, open': (
        (10, 0, 0, (14909440.0, 10436608.0), 59637760.0, '10528eb00e5c207c29248077c688ee2e6d692881a978acb27a4b3b3c2c944ac4'),
        (11, 0, 0, (14909440.0, 10436608.0), 59637760.0, 'c0c07d2fae6483e081dd15577ceec546196f83641579c2e72c1ff679f0d63cd4'),
        (11, 0, 0, (14909440.0, 10436608.0), 59637760.0, '2fba608e5f1dc07fc77ff569482252e8a3f620824ee4958226a121a5779e8bc5'),
    ),
    'contiguous, hyb': (
        (10, 0, 0, (11874304.0, 9318400.0), 47497216.0, 'c2ffa3d9252cf51d5b0d9f7854a65de6b0bb710c432d0f67466dee29b9e85a5b'),
        (11, 0, 0, (11874304.0, 9318400.0), 47497216.0, '28efa12121a0c19c4b6ec977fad72bee3f01ba6b6f3f1da3443c8a78f8290768'),
        (11, 0, 0, (11874304.0, 9318400.0), 47497216.0, '8a728b7351eb743a55ae2f030252a373aa64688e16664a805bd6393be1af1804'),
    ),
    'contiguous, symcols, closed form 1': (
        (10, 2, 0, (11874304.0, 9318400.0), 47497216.0, '5c6b9daa1f7f6c95119f4d927ae9b0932ae253a8d1da8925a5fa31cee1acd969'),
        (11, 4, 0, (11874304.0, 9318400.0), 47497216.0, '8826c118f4757d79d834c5f5db5d2ce6f652b9de51fcefaab09a9d9721f6750a'),
        (11, 6, 0, (11874304.0, 9318400.0), 47497216.0, '8fdebe2f5c75218349f36c65aef8c8173c9ce36f7df1e0c885a83e59640c8616'),
    ),
    'M = 96': (
        (8, 2, 0, (11796480.0, 8257536.0), 47185920.0, 'd19ecaa4253fd968f974dc93a330e95d478aa85eea7a846a1bdaccd3da16c884'),
        (9, 4, 0, (11796480.0, 8257536.0), 47185920.0, '413a5a922a32f2f1c46ef2cd87bda6c3e98acbbf1f25e95b6645a5e809e9e392'),
        (9, 6, 0, (11796480.0, 8257536.0), 47185920.0, '2f59e5431d3562b12d3533667f095e450685f08ff1c32f73bcdc5cb648f7bf32'),
    ),
    'M = 105': (
        (12, 0, 0, (0.0, 0.0), 0.0, '874ef94b7fafe3fff67fa371082ea12b3cbd298e46fca46180de82c54346b251'),
        (13, 0, 0, (0.0, 0.0), 0.0, '14ca7a6d9b95e5454b77dfb4e9c7e53e991d20c9d6bb0105865532167a6b0c20'),
        (13, 0, 0, (0.0, 0.0), 0.0, '23e53fe1094a800098e6133b086979e6905ce47a4da10f5ec1911228b7d2345a'),
    ),
    'n = 16': (
        (14, 0, 0, (6656000.0, 4659200.0), 26624000.0, 'bf79327a01be3c06d73e01da2d51d63312d23dca6cdba9f696f4b177f5be812d'),
        (15, 0, 0, (6656000.0, 4659200.0), 26624000.0, 'fcbf4b12af85fed123c07c12d4e50dc5b9037293cd5f91e3eb253a554cceec08'),
        (15, 0, 0, (6656000.0, 4659200.0), 26624000.0, 'e2256a6ccf9fe4fdadd16a14279300633782a842cc0397c16953e7e24e3e82c7'),
    ),
    'n = 33': (
        (16, 0, 0, (0.0, 0.0), 0.0, '23e5037c5cd5d2c9582ca46ef5e280993f3ac3518415f98c14d4cccd7a402f66'),
        (17, 0, 0, (0.0, 0.0), 0.0, '9b0982862efa4ad3df07aec998f741f8d6ccef0ca03ee5264a1457a91f17a72e'),
        (17, 0, 0, (0.0, 0.0), 0.0, '912f845085d0a8ac642f4d163f80646d27e7e21424affc96f192c783e3b1b14c'),
    ),
    'M = 96, 33 walkers': (
        (8, 31, 0, (11796480.0, 8257536.0), 389283840.0, '796b0e7585da1261c4387d93c62f7b6d8eed9530db2440f79b128b2009d537e9'),
        (9, 62, 0, (11796480.0, 8257536.0), 389283840.0, '4be8bda7ce237f012fffc72c6e869d859b550413dffd478455a83156638840fc'),
        (9, 93, 0, (11796480.0, 8257536.0), 389283840.0, '3f2a7b4f2b6deaf3f290741e193cb6e2b3ddc4376e347ce1cc7091c3e32bf435'),
    ),
    'M = 105, 33 walkers': (
        (12, 0, 0, (0.0, 0.0), 0.0, 'c37ad95b205c31f83fda56956b76eb499c22d1e0efbf2bc85aa937853fd9f443'),
        (13, 0, 0, (0.0, 0.0), 0.0, '752d20e49888b7fd46050b1e06f89f93e5596869c3bcbb935fa9b85a32ea5b9d'),
        (13, 0, 0, (0.0, 0.0), 0.0, 'bac23c3c3f0f5e649835bdb978fda840ae16f7a9347d24d50d78cb5cb669e932'),
    ),
    'n = 16, 33 walkers': (
        (14, 0, 0, (6656000.0, 4659200.0), 219648000.0, '232512e1cfc3bb4d2f1e21ca94e94e75ee62c4948909c1bf54ef6ca85736a811'),
        (15, 0, 0, (6656000.0, 4659200.0), 219648000.0, '1690917a6c3fecca9ae4605dca0e2822806ffc81bc2e805e7ff989b584f4fcc8'),
        (15, 0, 0, (6656000.0, 4659200.0), 219648000.0, 'a8653f58ee3e09fdfb60e00912cf0efb92204032101e5e0bc3b8e5e08e6d0549'),
    ),
    'n = 33, 33 walkers': (
        (16, 0, 0, (0.0, 0.0), 0.0, '2f3165bb47b17c1c195ab005f2809da5a405e86943010f6cec108a70f5de68c8'),
        (17, 0, 0, (0.0, 0.0), 0.0, '6e2c203668986c0ec04de376731e5cd289f314a1be8b365bb86cd3b3a93e7727'),
        (17, 0, 0, (0.0, 0.0), 0.0, '0df5805e32db96883188c6f5d3237bb9598c251b4a715d91318985e2c6fa7b04'),
    ),
    'complex BH1': (
        (10, 2, 0, (14536704.0, 11980800.0), 58146816.0, '4aad91c5c4670be6aed40115e9411102c46dee768ce62353c086f1f351f95d91'),
        (11, 4, 0, (14536704.0, 11980800.0), 58146816.0, '510e7250e4b90bafe32d3392e20ad75577cdb599049fb2e35b83e6907e6a14b5'),
        (11, 6, 0, (14536704.0, 11980800.0), 58146816.0, '22071c84988f486fecef89c0ee445180f39c5643264d3c1f2bba820f73b7fc97'),
    ),
    'spin-dependent BH1': (
        (10, 0, 0, (13312000.0, 9318400.0), 53248000.0, '1b538e184cde4ae300122c4f16929d80c251da35e376bf5aa8924d4bc8115c2b'),
        (11, 0, 0, (13312000.0, 9318400.0), 53248000.0, 'e1ae82ef6b3333012d4b49187fb1fa837980dcf01a7c7127edcdba2d169f7063'),
        (11, 0, 0, (13312000.0, 9318400.0), 53248000.0, '9e6e56187e549c3d2fec3ced03399254a46254def24c52ea6c2fa6ca81345850'),
    ),
    'complex BH1, 33 walkers': (
        (10, 31, 0, (14536704.0, 11980800.0), 479711232.0, '573ac12ceb0e30d31787f2920b984ad7184789f6f1d0599119542016b141ac67'),
        (11, 62, 0, (14536704.0, 11980800.0), 479711232.0, '394f967bbf416a8d10224a6b7fbef85ff48422e66695b41fa5c6befb678fda17'),
        (11, 93, 0, (14536704.0, 11980800.0), 479711232.0, '54d65d9df0f2bee8d388203835a30fd27b32f121fdcb0e5e9ec679cddb5426e9'),
    ),
    'spin-dependent BH1, 33 walkers': (
        (10, 0, 0, (13312000.0, 9318400.0), 439296000.0, 'd40266eb618167331116f85447e0fd1e973af737a869926b023ac0f98a4d026c'),
        (11, 0, 0, (13312000.0, 9318400.0), 439296000.0, 'fb080296beb60b2b79723bde818e1847897114fe6d9f8fcf2667ea0d42230796'),
        (11, 0, 0, (13312000.0, 9318400.0), 439296000.0, '4f6fc22ed267fcce03ccac1b6ff75d47539e1ad4d63f57e88d628422e5a8700d'),
    ),
    'resident 97, 17': (
        (10, 2, 0, (13312000.0, 8601600.0), 53248000.0, '873436783331314299c5d5301c649a085785d2ee784d20038474d5c713aefc23'),
        (11, 4, 0, (13312000.0, 8601600.0), 53248000.0, 'fb4d97a9bd6274a94c6086ba86eacf488d60fdf4217cd12bb2ddafde6ad1fa9d'),
        (11, 6, 0, (13312000.0, 8601600.0), 53248000.0, 'b3ccfea36dcd9a43d1cbc06fa0e6120791de3c04dc6a264411772734325fadfc'),
    ),
    'resident 100, 25': (
        (10, 2, 0, (11874304.0, 8601600.0), 47497216.0, '96aed5239466933f516a9272cc96f21a30b8924a1ba3129e9bc27807a39f82c7'),
        (11, 4, 0, (11874304.0, 8601600.0), 47497216.0, '2e0ac721b444575b6d66a7e7990a8809cdbe11ad62a2d81f6830dc5ff02c0833'),
        (11, 6, 0, (11874304.0, 8601600.0), 47497216.0, '160a72b71db8d69753853a76c68739e3059fef76a92ea3a545e7faa90973cfb8'),
    ),
    'resident 104, 32': (
        (10, 2, 0, (14909440.0, 8945664.0), 59637760.0, 'ee585c1a9607c56198e7b120b7f237b6b44e11aae6d4ff6738be6217b6be4cac'),
        (11, 4, 0, (14909440.0, 8945664.0), 59637760.0, '213b82632fb6f68ed2a89038eb89addb5d7283b643081422dfa2fab51f16fb46'),
        (11, 6, 0, (14909440.0, 8945664.0), 59637760.0, 'ba4827a0b6d62ca449814fcad61ba7a6e891ab4fdd55bc7fd6f444463a6618d5'),
    ),
    'resident 97, 17: fusion 0 scope 0 overlap 1 hand-over 1': (
        (10, 31, 0, (13312000.0, 8601600.0), 439296000.0, '7985df18f51292186e886a3e98a6a19c3937338fa01e3eb875c125c9d1878a3d'),
        (11, 62, 0, (13312000.0, 8601600.0), 439296000.0, '1a7feb81e6344221a4e94183dcd33bf92eec3bddaf0a7fc8c10180836d72d99d'),
        (11, 93, 0, (13312000.0, 8601600.0), 439296000.0, '62241a001b6c7cb83372857c81244b09b595f8d879f0a626741f7412cd8be7a5'),
    ),
    'resident 97, 17: fusion 0 scope 0 overlap 1 hand-over 0': (
        (10, 31, 0, (13312000.0, 8601600.0), 439296000.0, '7985df18f51292186e886a3e98a6a19c3937338fa01e3eb875c125c9d1878a3d'),
        (11, 62, 0, (13312000.0, 8601600.0), 439296000.0, '1a7feb81e6344221a4e94183dcd33bf92eec3bddaf0a7fc8c10180836d72d99d'),
        (11, 93, 0, (13312000.0, 8601600.0), 439296000.0, '62241a001b6c7cb83372857c81244b09b595f8d879f0a626741f7412cd8be7a5'),
    ),
    'resident 97, 17: fusion 0 scope 0 overlap 0 hand-over 0': (
        (10, 31, 0, (13312000.0, 8601600.0), 439296000.0, '7985df18f51292186e886a3e98a6a19c3937338fa01e3eb875c125c9d1878a3d'),
        (11, 62, 0, (13312000.0, 8601600.0), 439296000.0, '1a7feb81e6344221a4e94183dcd33bf92eec3bddaf0a7fc8c10180836d72d99d'),
        (11, 93, 0, (13312000.0, 8601600.0), 439296000.0, '62241a001b6c7cb83372857c81244b09b595f8d879f0a626741f7412cd8be7a5'),
    ),
    'resident 97, 17: fusion 0 scope 1 overlap 1 hand-over 1': (
        (10, 31, 0, (13312000.0, 8601600.0), 439296000.0, '7985df18f51292186e886a3e98a6a19c3937338fa01e3eb875c125c9d1878a3d'),
        (11, 62, 0, (13312000.0, 8601600.0), 439296000.0, '1a7feb81e6344221a4e94183dcd33bf92eec3bddaf0a7fc8c10180836d72d99d'),
        (11, 93, 0, (13312000.0, 8601600.0), 439296000.0, '62241a001b6c7cb83372857c81244b09b595f8d879f0a626741f7412cd8be7a5'),
    ),
    'resident 97, 17: fusion 0 scope 1 overlap 1 hand-over 0': (
        (10, 31, 0, (13312000.0, 8601600.0), 439296000.0, '7985df18f51292186e886a3e98a6a19c3937338fa01e3eb875c125c9d1878a3d'),
        (11, 62, 0, (13312000.0, 8601600.0), 439296000.0, '1a7feb81e6344221a4e94183dcd33bf92eec3bddaf0a7fc8c10180836d72d99d'),
        (11, 93, 0, (13312000.0, 8601600.0), 439296000.0, '62241a001b6c7cb83372857c81244b09b595f8d879f0a626741f7412cd8be7a5'),
    ),
    'resident 97, 17: fusion 0 scope 1 overlap 0 hand-over 0': (
        (10, 31, 0, (13312000.0, 8601600.0), 439296000.0, '7985df18f51292186e886a3e98a6a19c3937338fa01e3eb875c125c9d1878a3d'),
        (11, 62, 0, (13312000.0, 8601600.0), 439296000.0, '1a7feb81e6344221a4e94183dcd33bf92eec3bddaf0a7fc8c10180836d72d99d'),
        (11, 93, 0, (13312000.0, 8601600.0), 439296000.0, '62241a001b6c7cb83372857c81244b09b595f8d879f0a626741f7412cd8be7a5'),
    ),
    'resident 97, 17: fusion 1 scope 0 overlap 1 hand-over 1': (
        (18, 31, 0, (15089664.0, 9490432.0), 497958912.0, '7985df18f51292186e886a3e98a6a19c3937338fa01e3eb875c125c9d1878a3d'),
        (11, 62, 0, (13312000.0, 8601600.0), 439296000.0, '1a7feb81e6344221a4e94183dcd33bf92eec3bddaf0a7fc8c10180836d72d99d'),
        (19, 93, 0, (15089664.0, 9490432.0), 497958912.0, '62241a001b6c7cb83372857c81244b09b595f8d879f0a626741f7412cd8be7a5'),
    ),
    'resident 97, 17: fusion 1 scope 0 overlap 1 hand-over 0': (
        (18, 31, 0, (15089664.0, 9490432.0), 497958912.0, '7985df18f51292186e886a3e98a6a19c3937338fa01e3eb875c125c9d1878a3d'),
        (11, 62, 0, (13312000.0, 8601600.0), 439296000.0, '1a7feb81e6344221a4e94183dcd33bf92eec3bddaf0a7fc8c10180836d72d99d'),
        (19, 93, 0, (15089664.0, 9490432.0), 497958912.0, '62241a001b6c7cb83372857c81244b09b595f8d879f0a626741f7412cd8be7a5'),
    ),
    'resident 97, 17: fusion 1 scope 0 overlap 0 hand-over 0': (
        (18, 31, 0, (15089664.0, 9490432.0), 497958912.0, '7985df18f51292186e886a3e98a6a19c3937338fa01e3eb875c125c9d1878a3d'),
        (11, 62, 0, (13312000.0, 8601600.0), 439296000.0, '1a7feb81e6344221a4e94183dcd33bf92eec3bddaf0a7fc8c10180836d72d99d'),
        (19, 93, 0, (15089664.0, 9490432.0), 497958912.0, '62241a001b6c7cb83372857c81244b09b595f8d879f0a626741f7412cd8be7a5'),
    ),
    'resident 97, 17: fusion 1 scope 1 overlap 1 hand-over 1': (
        (18, 31, 0, (15089664.0, 9490432.0), 497958912.0, '7985df18f51292186e886a3e98a6a19c3937338fa01e3eb875c125c9d1878a3d'),
        (19, 62, 0, (15089664.0, 9490432.0), 497958912.0, '1a7feb81e6344221a4e94183dcd33bf92eec3bddaf0a7fc8c10180836d72d99d'),
        (19, 93, 0, (15089664.0, 9490432.0), 497958912.0, '62241a001b6c7cb83372857c81244b09b595f8d879f0a626741f7412cd8be7a5'),
    ),
    'resident 97, 17: fusion 1 scope 1 overlap 1 hand-over 0': (
        (18, 31, 0, (15089664.0, 9490432.0), 497958912.0, '7985df18f51292186e886a3e98a6a19c3937338fa01e3eb875c125c9d1878a3d'),
        (19, 62, 0, (15089664.0, 9490432.0), 497958912.0, '1a7feb81e6344221a4e94183dcd33bf92eec3bddaf0a7fc8c10180836d72d99d'),
        (19, 93, 0, (15089664.0, 9490432.0), 497958912.0, '62241a001b6c7cb83372857c81244b09b595f8d879f0a626741f7412cd8be7a5'),
    ),
    'resident 97, 17: fusion 1 scope 1 overlap 0 hand-over 0': (
        (18, 31, 0, (15089664.0, 9490432.0), 497958912.0, '7985df18f51292186e886a3e98a6a19c3937338fa01e3eb875c125c9d1878a3d'),
        (19, 62, 0, (15089664.0, 9490432.0), 497958912.0, '1a7feb81e6344221a4e94183dcd33bf92eec3bddaf0a7fc8c10180836d72d99d'),
        (19, 93, 0, (15089664.0, 9490432.0), 497958912.0, '62241a001b6c7cb83372857c81244b09b595f8d879f0a626741f7412cd8be7a5'),
    ),
    'resident 97, 17: fusion 2 scope 0 overlap 1 hand-over 1': (
        (20, 31, 0, (15089664.0, 9441280.0), 497958912.0, '7793f1902b39f6826858e5020dfd557d90852a4fdfa679a45d7e73b7e8cfd3db'),
        (11, 62, 0, (13312000.0, 8601600.0), 439296000.0, '03098830b296cd1b6e8dea5bf31363e46b59a89fef0d771c6a00cd401cdfccf4'),
        (21, 93, 0, (15089664.0, 9441280.0), 497958912.0, '930faafdabef9af78616ef3876eec632ccea696c7c4bbe364c490bcb91bd9c88'),
    ),
    'resident 97, 17: fusion 2 scope 0 overlap 1 hand-over 0': (
        (20, 31, 0, (15089664.0, 8007680.0), 497958912.0, '7793f1902b39f6826858e5020dfd557d90852a4fdfa679a45d7e73b7e8cfd3db'),
        (11, 62, 0, (13312000.0, 8601600.0), 439296000.0, '03098830b296cd1b6e8dea5bf31363e46b59a89fef0d771c6a00cd401cdfccf4'),
        (21, 93, 0, (15089664.0, 8007680.0), 497958912.0, '930faafdabef9af78616ef3876eec632ccea696c7c4bbe364c490bcb91bd9c88'),
    ),
    'resident 97, 17: fusion 2 scope 0 overlap 0 hand-over 0': (
        (20, 31, 0, (15089664.0, 8056832.0), 497958912.0, '448ffbcd2e22090b15d630924ec34d20d96e97be104da83c1f67a0e02346ad29'),
        (11, 62, 0, (13312000.0, 8601600.0), 439296000.0, 'eb71b431e1bad3aaded37679a5561576d14a734ef817f0e15137c1ef7ac9b5f9'),
        (21, 93, 0, (15089664.0, 8056832.0), 497958912.0, 'e655f83fc1e623f66371a8a436493de2347aded3f65ecb092e66441b3db1678e'),
    ),
    'resident 97, 17: fusion 2 scope 1 overlap 1 hand-over 1': (
        (20, 31, 0, (15089664.0, 9441280.0), 497958912.0, '7793f1902b39f6826858e5020dfd557d90852a4fdfa679a45d7e73b7e8cfd3db'),
        (21, 62, 31, (15089664.0, 8007680.0), 497958912.0, 'b2b847c48a48fdb8e7d5fc1044b8247a497fc82ecafe4c4a946943248e5359b9'),
        (21, 93, 62, (15089664.0, 8007680.0), 497958912.0, '6246208c25dbbf090f908eea1747bc497c15a3b117bba5e6ff2cb4cdedd488a8'),
    ),
    'resident 97, 17: fusion 2 scope 1 overlap 1 hand-over 0': (
        (20, 31, 0, (15089664.0, 8007680.0), 497958912.0, '7793f1902b39f6826858e5020dfd557d90852a4fdfa679a45d7e73b7e8cfd3db'),
        (21, 62, 0, (15089664.0, 8007680.0), 497958912.0, '81cee970f3540ae046a5496a43bbb67df7a94b6c8bc5fb1ad6efc0195923729e'),
        (21, 93, 0, (15089664.0, 8007680.0), 497958912.0, '1b493e0dd99e5a2821a2726ae30dff826c89b5824a848732539f0be70192a9f1'),
    ),
    'resident 97, 17: fusion 2 scope 1 overlap 0 hand-over 0': (
        (20, 31, 0, (15089664.0, 8056832.0), 497958912.0, '448ffbcd2e22090b15d630924ec34d20d96e97be104da83c1f67a0e02346ad29'),
        (21, 62, 0, (15089664.0, 8056832.0), 497958912.0, '609dbe927e2c476e2cd241307a89428d22c9049f94b8c9168c75b61f49648612'),
        (21, 93, 0, (15089664.0, 8056832.0), 497958912.0, 'bc5367a9649778ebfaf365b6a372a5968e402032f79230ae572e682f3f8f2c79'),
    ),
    'resident 100, 25: fusion 0 scope 0 overlap 1 hand-over 1': (
        (10, 31, 0, (11874304.0, 8601600.0), 391852032.0, 'd0dba464e212fd10c693f7e94cac3b67c973bb38e231fe1bc892fd3684a7d822'),
        (11, 62, 0, (11874304.0, 8601600.0), 391852032.0, '5a315bcc860c1c91bd10ef9974f2f262bf7c4dcc34f2d8b3094c08e19cd5386e'),
        (11, 93, 0, (11874304.0, 8601600.0), 391852032.0, 'bf053903aae9df7d95245ff0a3ac484f7850233401ab8d6edd0303797aeb9c52'),
    ),
    'resident 100, 25: fusion 0 scope 0 overlap 1 hand-over 0': (
        (10, 31, 0, (11874304.0, 8601600.0), 391852032.0, 'd0dba464e212fd10c693f7e94cac3b67c973bb38e231fe1bc892fd3684a7d822'),
        (11, 62, 0, (11874304.0, 8601600.0), 391852032.0, '5a315bcc860c1c91bd10ef9974f2f262bf7c4dcc34f2d8b3094c08e19cd5386e'),
        (11, 93, 0, (11874304.0, 8601600.0), 391852032.0, 'bf053903aae9df7d95245ff0a3ac484f7850233401ab8d6edd0303797aeb9c52'),
    ),
    'resident 100, 25: fusion 0 scope 0 overlap 0 hand-over 0': (
        (10, 31, 0, (11874304.0, 8601600.0), 391852032.0, 'd0dba464e212fd10c693f7e94cac3b67c973bb38e231fe1bc892fd3684a7d822'),
        (11, 62, 0, (11874304.0, 8601600.0), 391852032.0, '5a315bcc860c1c91bd10ef9974f2f262bf7c4dcc34f2d8b3094c08e19cd5386e'),
        (11, 93, 0, (11874304.0, 8601600.0), 391852032.0, 'bf053903aae9df7d95245ff0a3ac484f7850233401ab8d6edd0303797aeb9c52'),
    ),
    'resident 100, 25: fusion 0 scope 1 overlap 1 hand-over 1': (
        (10, 31, 0, (11874304.0, 8601600.0), 391852032.0, 'd0dba464e212fd10c693f7e94cac3b67c973bb38e231fe1bc892fd3684a7d822'),
        (11, 62, 0, (11874304.0, 8601600.0), 391852032.0, '5a315bcc860c1c91bd10ef9974f2f262bf7c4dcc34f2d8b3094c08e19cd5386e'),
        (11, 93, 0, (11874304.0, 8601600.0), 391852032.0, 'bf053903aae9df7d95245ff0a3ac484f7850233401ab8d6edd0303797aeb9c52'),
    ),
    'resident 100, 25: fusion 0 scope 1 overlap 1 hand-over 0': (
        (10, 31, 0, (11874304.0, 8601600.0), 391852032.0, 'd0dba464e212fd10c693f7e94cac3b67c973bb38e231fe1bc892fd3684a7d822'),
        (11, 62, 0, (11874304.0, 8601600.0), 391852032.0, '5a315bcc860c1c91bd10ef9974f2f262bf7c4dcc34f2d8b3094c08e19cd5386e'),
        (11, 93, 0, (11874304.0, 8601600.0), 391852032.0, 'bf053903aae9df7d95245ff0a3ac484f7850233401ab8d6edd0303797aeb9c52'),
    ),
    'resident 100, 25: fusion 0 scope 1 overlap 0 hand-over 0': (
        (10, 31, 0, (11874304.0, 8601600.0), 391852032.0, 'd0dba464e212fd10c693f7e94cac3b67c973bb38e231fe1bc892fd3684a7d822'),
        (11, 62, 0, (11874304.0, 8601600.0), 391852032.0, '5a315bcc860c1c91bd10ef9974f2f262bf7c4dcc34f2d8b3094c08e19cd5386e'),
        (11, 93, 0, (11874304.0, 8601600.0), 391852032.0, 'bf053903aae9df7d95245ff0a3ac484f7850233401ab8d6edd0303797aeb9c52'),
    ),
    'resident 100, 25: fusion 1 scope 0 overlap 1 hand-over 1': (
        (18, 31, 0, (13996032.0, 9662464.0), 461869056.0, 'd0dba464e212fd10c693f7e94cac3b67c973bb38e231fe1bc892fd3684a7d822'),
        (11, 62, 0, (11874304.0, 8601600.0), 391852032.0, '5a315bcc860c1c91bd10ef9974f2f262bf7c4dcc34f2d8b3094c08e19cd5386e'),
        (19, 93, 0, (13996032.0, 9662464.0), 461869056.0, 'bf053903aae9df7d95245ff0a3ac484f7850233401ab8d6edd0303797aeb9c52'),
    ),
    'resident 100, 25: fusion 1 scope 0 overlap 1 hand-over 0': (
        (18, 31, 0, (13996032.0, 9662464.0), 461869056.0, 'd0dba464e212fd10c693f7e94cac3b67c973bb38e231fe1bc892fd3684a7d822'),
        (11, 62, 0, (11874304.0, 8601600.0), 391852032.0, '5a315bcc860c1c91bd10ef9974f2f262bf7c4dcc34f2d8b3094c08e19cd5386e'),
        (19, 93, 0, (13996032.0, 9662464.0), 461869056.0, 'bf053903aae9df7d95245ff0a3ac484f7850233401ab8d6edd0303797aeb9c52'),
    ),
    'resident 100, 25: fusion 1 scope 0 overlap 0 hand-over 0': (
        (18, 31, 0, (13996032.0, 9662464.0), 461869056.0, 'd0dba464e212fd10c693f7e94cac3b67c973bb38e231fe1bc892fd3684a7d822'),
        (11, 62, 0, (11874304.0, 8601600.0), 391852032.0, '5a315bcc860c1c91bd10ef9974f2f262bf7c4dcc34f2d8b3094c08e19cd5386e'),
        (19, 93, 0, (13996032.0, 9662464.0), 461869056.0, 'bf053903aae9df7d95245ff0a3ac484f7850233401ab8d6edd0303797aeb9c52'),
    ),
    'resident 100, 25: fusion 1 scope 1 overlap 1 hand-over 1': (
        (18, 31, 0, (13996032.0, 9662464.0), 461869056.0, 'd0dba464e212fd10c693f7e94cac3b67c973bb38e231fe1bc892fd3684a7d822'),
        (19, 62, 0, (13996032.0, 9662464.0), 461869056.0, '5a315bcc860c1c91bd10ef9974f2f262bf7c4dcc34f2d8b3094c08e19cd5386e'),
        (19, 93, 0, (13996032.0, 9662464.0), 461869056.0, 'bf053903aae9df7d95245ff0a3ac484f7850233401ab8d6edd0303797aeb9c52'),
    ),
    'resident 100, 25: fusion 1 scope 1 overlap 1 hand-over 0': (
        (18, 31, 0, (13996032.0, 9662464.0), 461869056.0, 'd0dba464e212fd10c693f7e94cac3b67c973bb38e231fe1bc892fd3684a7d822'),
        (19, 62, 0, (13996032.0, 9662464.0), 461869056.0, '5a315bcc860c1c91bd10ef9974f2f262bf7c4dcc34f2d8b3094c08e19cd5386e'),
        (19, 93, 0, (13996032.0, 9662464.0), 461869056.0, 'bf053903aae9df7d95245ff0a3ac484f7850233401ab8d6edd0303797aeb9c52'),
    ),
    'resident 100, 25: fusion 1 scope 1 overlap 0 hand-over 0': (
        (18, 31, 0, (13996032.0, 9662464.0), 461869056.0, 'd0dba464e212fd10c693f7e94cac3b67c973bb38e231fe1bc892fd3684a7d822'),
        (19, 62, 0, (13996032.0, 9662464.0), 461869056.0, '5a315bcc860c1c91bd10ef9974f2f262bf7c4dcc34f2d8b3094c08e19cd5386e'),
        (19, 93, 0, (13996032.0, 9662464.0), 461869056.0, 'bf053903aae9df7d95245ff0a3ac484f7850233401ab8d6edd0303797aeb9c52'),
    ),
    'resident 100, 25: fusion 2 scope 0 overlap 1 hand-over 1': (
        (20, 31, 0, (13996032.0, 9613312.0), 461869056.0, 'a213038d01fc3e09f6ee099007005b878c15a72fc0d49e9dc94515680a52ab2a'),
        (11, 62, 0, (11874304.0, 8601600.0), 391852032.0, 'e2295d4c26b29d76a1aab541cc56baaad1d01e4ba927382ef7d6efe6e49b35c9'),
        (21, 93, 0, (13996032.0, 9613312.0), 461869056.0, 'd06b8a6d21f30776600b4a03dee00ddfa9f2960141da180e47822d887f74b9dd'),
    ),
    'resident 100, 25: fusion 2 scope 0 overlap 1 hand-over 0': (
        (20, 31, 0, (13996032.0, 8179712.0), 461869056.0, 'a213038d01fc3e09f6ee099007005b878c15a72fc0d49e9dc94515680a52ab2a'),
        (11, 62, 0, (11874304.0, 8601600.0), 391852032.0, 'e2295d4c26b29d76a1aab541cc56baaad1d01e4ba927382ef7d6efe6e49b35c9'),
        (21, 93, 0, (13996032.0, 8179712.0), 461869056.0, 'd06b8a6d21f30776600b4a03dee00ddfa9f2960141da180e47822d887f74b9dd'),
    ),
    'resident 100, 25: fusion 2 scope 0 overlap 0 hand-over 0': (
        (20, 31, 0, (13996032.0, 8228864.0), 461869056.0, 'dd4f6e09c63cda774bd1c740f3df28e778f6043179d6ab9df595d8c930145b29'),
        (11, 62, 0, (11874304.0, 8601600.0), 391852032.0, '47b453e35351c691df2fdb64cd8337790ea9f73491a4cb982366ea31bae31214'),
        (21, 93, 0, (13996032.0, 8228864.0), 461869056.0, 'd2196178ed6f2103aef3b0b1946e32ea02eacbb0387cd5b4c84afad7392a5af3'),
    ),
    'resident 100, 25: fusion 2 scope 1 overlap 1 hand-over 1': (
        (20, 31, 0, (13996032.0, 9613312.0), 461869056.0, 'a213038d01fc3e09f6ee099007005b878c15a72fc0d49e9dc94515680a52ab2a'),
        (21, 62, 31, (13996032.0, 8179712.0), 461869056.0, 'd15cf40b40f5749cb950dc4b9a03fa2a7a2e288b2d0f6c72840f3ed88c7c5e92'),
        (21, 93, 62, (13996032.0, 8179712.0), 461869056.0, '4f25c9356fd7beac7c4ea0c5f58c7e3f5e0020fb50da698d00fb3941b7a326ec'),
    ),
    'resident 100, 25: fusion 2 scope 1 overlap 1 hand-over 0': (
        (20, 31, 0, (13996032.0, 8179712.0), 461869056.0, 'a213038d01fc3e09f6ee099007005b878c15a72fc0d49e9dc94515680a52ab2a'),
        (21, 62, 0, (13996032.0, 8179712.0), 461869056.0, 'f71bfd36dc759e704d7f5af60fd40003c53a595861e0c44f4a19f501a1f8530d'),
        (21, 93, 0, (13996032.0, 8179712.0), 461869056.0, 'c469f676bf7c89a9d5134adafd16858320f387064bae626d24849bb830dceeb5'),
    ),
    'resident 100, 25: fusion 2 scope 1 overlap 0 hand-over 0': (
        (20, 31, 0, (13996032.0, 8228864.0), 461869056.0, 'dd4f6e09c63cda774bd1c740f3df28e778f6043179d6ab9df595d8c930145b29'),
        (21, 62, 0, (13996032.0, 8228864.0), 461869056.0, 'fb16c0b2e63aa3e3036da2cee1475895a575d5eabbfc2bf99a5c6ebad132d44a'),
        (21, 93, 0, (13996032.0, 8228864.0), 461869056.0, 'e2945d1eeee42f2e94f853634ea30068093e79be4ddd7dafd2d109379b346fd7'),
    ),
    'resident 104, 32: fusion 0 scope 0 overlap 1 hand-over 1': (
        (10, 31, 0, (14909440.0, 8945664.0), 492011520.0, 'ff520ae6a88783486e1f624ec8a51b497cdff400b0f50ee8eda6468f2e4e3b53'),
        (11, 62, 0, (14909440.0, 8945664.0), 492011520.0, 'f564850dfdc02d5058492cea8fcd5261ac4360d8155ce31c0d42b86a634ea05e'),
        (11, 93, 0, (14909440.0, 8945664.0), 492011520.0, '613eaa9ef216343ba59f70b5efeacf7ae1a972f1d81f21751e5275e370fd9e4d'),
    ),
    'resident 104, 32: fusion 0 scope 0 overlap 1 hand-over 0': (
        (10, 31, 0, (14909440.0, 8945664.0), 492011520.0, 'ff520ae6a88783486e1f624ec8a51b497cdff400b0f50ee8eda6468f2e4e3b53'),
        (11, 62, 0, (14909440.0, 8945664.0), 492011520.0, 'f564850dfdc02d5058492cea8fcd5261ac4360d8155ce31c0d42b86a634ea05e'),
        (11, 93, 0, (14909440.0, 8945664.0), 492011520.0, '613eaa9ef216343ba59f70b5efeacf7ae1a972f1d81f21751e5275e370fd9e4d'),
    ),
    'resident 104, 32: fusion 0 scope 0 overlap 0 hand-over 0': (
        (10, 31, 0, (14909440.0, 8945664.0), 492011520.0, 'ff520ae6a88783486e1f624ec8a51b497cdff400b0f50ee8eda6468f2e4e3b53'),
        (11, 62, 0, (14909440.0, 8945664.0), 492011520.0, 'f564850dfdc02d5058492cea8fcd5261ac4360d8155ce31c0d42b86a634ea05e'),
        (11, 93, 0, (14909440.0, 8945664.0), 492011520.0, '613eaa9ef216343ba59f70b5efeacf7ae1a972f1d81f21751e5275e370fd9e4d'),
    ),
    'resident 104, 32: fusion 0 scope 1 overlap 1 hand-over 1': (
        (10, 31, 0, (14909440.0, 8945664.0), 492011520.0, 'ff520ae6a88783486e1f624ec8a51b497cdff400b0f50ee8eda6468f2e4e3b53'),
        (11, 62, 0, (14909440.0, 8945664.0), 492011520.0, 'f564850dfdc02d5058492cea8fcd5261ac4360d8155ce31c0d42b86a634ea05e'),
        (11, 93, 0, (14909440.0, 8945664.0), 492011520.0, '613eaa9ef216343ba59f70b5efeacf7ae1a972f1d81f21751e5275e370fd9e4d'),
    ),
    'resident 104, 32: fusion 0 scope 1 overlap 1 hand-over 0': (
        (10, 31, 0, (14909440.0, 8945664.0), 492011520.0, 'ff520ae6a88783486e1f624ec8a51b497cdff400b0f50ee8eda6468f2e4e3b53'),
        (11, 62, 0, (14909440.0, 8945664.0), 492011520.0, 'f564850dfdc02d5058492cea8fcd5261ac4360d8155ce31c0d42b86a634ea05e'),
        (11, 93, 0, (14909440.0, 8945664.0), 492011520.0, '613eaa9ef216343ba59f70b5efeacf7ae1a972f1d81f21751e5275e370fd9e4d'),
    ),
    'resident 104, 32: fusion 0 scope 1 overlap 0 hand-over 0': (
        (10, 31, 0, (14909440.0, 8945664.0), 492011520.0, 'ff520ae6a88783486e1f624ec8a51b497cdff400b0f50ee8eda6468f2e4e3b53'),
        (11, 62, 0, (14909440.0, 8945664.0), 492011520.0, 'f564850dfdc02d5058492cea8fcd5261ac4360d8155ce31c0d42b86a634ea05e'),
        (11, 93, 0, (14909440.0, 8945664.0), 492011520.0, '613eaa9ef216343ba59f70b5efeacf7ae1a972f1d81f21751e5275e370fd9e4d'),
    ),
    'resident 104, 32: fusion 1 scope 0 overlap 1 hand-over 1': (
        (18, 31, 0, (17203200.0, 10092544.0), 567705600.0, 'ff520ae6a88783486e1f624ec8a51b497cdff400b0f50ee8eda6468f2e4e3b53'),
        (11, 62, 0, (14909440.0, 8945664.0), 492011520.0, 'f564850dfdc02d5058492cea8fcd5261ac4360d8155ce31c0d42b86a634ea05e'),
        (19, 93, 0, (17203200.0, 10092544.0), 567705600.0, '613eaa9ef216343ba59f70b5efeacf7ae1a972f1d81f21751e5275e370fd9e4d'),
    ),
    'resident 104, 32: fusion 1 scope 0 overlap 1 hand-over 0': (
        (18, 31, 0, (17203200.0, 10092544.0), 567705600.0, 'ff520ae6a88783486e1f624ec8a51b497cdff400b0f50ee8eda6468f2e4e3b53'),
        (11, 62, 0, (14909440.0, 8945664.0), 492011520.0, 'f564850dfdc02d5058492cea8fcd5261ac4360d8155ce31c0d42b86a634ea05e'),
        (19, 93, 0, (17203200.0, 10092544.0), 567705600.0, '613eaa9ef216343ba59f70b5efeacf7ae1a972f1d81f21751e5275e370fd9e4d'),
    ),
    'resident 104, 32: fusion 1 scope 0 overlap 0 hand-over 0': (
        (18, 31, 0, (17203200.0, 10092544.0), 567705600.0, 'ff520ae6a88783486e1f624ec8a51b497cdff400b0f50ee8eda6468f2e4e3b53'),
        (11, 62, 0, (14909440.0, 8945664.0), 492011520.0, 'f564850dfdc02d5058492cea8fcd5261ac4360d8155ce31c0d42b86a634ea05e'),
        (19, 93, 0, (17203200.0, 10092544.0), 567705600.0, '613eaa9ef216343ba59f70b5efeacf7ae1a972f1d81f21751e5275e370fd9e4d'),
    ),
    'resident 104, 32: fusion 1 scope 1 overlap 1 hand-over 1': (
        (18, 31, 0, (17203200.0, 10092544.0), 567705600.0, 'ff520ae6a88783486e1f624ec8a51b497cdff400b0f50ee8eda6468f2e4e3b53'),
        (19, 62, 0, (17203200.0, 10092544.0), 567705600.0, 'f564850dfdc02d5058492cea8fcd5261ac4360d8155ce31c0d42b86a634ea05e'),
        (19, 93, 0, (17203200.0, 10092544.0), 567705600.0, '613eaa9ef216343ba59f70b5efeacf7ae1a972f1d81f21751e5275e370fd9e4d'),
    ),
    'resident 104, 32: fusion 1 scope 1 overlap 1 hand-over 0': (
        (18, 31, 0, (17203200.0, 10092544.0), 567705600.0, 'ff520ae6a88783486e1f624ec8a51b497cdff400b0f50ee8eda6468f2e4e3b53'),
        (19, 62, 0, (17203200.0, 10092544.0), 567705600.0, 'f564850dfdc02d5058492cea8fcd5261ac4360d8155ce31c0d42b86a634ea05e'),
        (19, 93, 0, (17203200.0, 10092544.0), 567705600.0, '613eaa9ef216343ba59f70b5efeacf7ae1a972f1d81f21751e5275e370fd9e4d'),
    ),
    'resident 104, 32: fusion 1 scope 1 overlap 0 hand-over 0': (
        (18, 31, 0, (17203200.0, 10092544.0), 567705600.0, 'ff520ae6a88783486e1f624ec8a51b497cdff400b0f50ee8eda6468f2e4e3b53'),
        (19, 62, 0, (17203200.0, 10092544.0), 567705600.0, 'f564850dfdc02d5058492cea8fcd5261ac4360d8155ce31c0d42b86a634ea05e'),
        (19, 93, 0, (17203200.0, 10092544.0), 567705600.0, '613eaa9ef216343ba59f70b5efeacf7ae1a972f1d81f21751e5275e370fd9e4d'),
    ),
    'resident 104, 32: fusion 2 scope 0 overlap 1 hand-over 1': (
        (20, 31, 0, (17203200.0, 10059776.0), 567705600.0, 'f117a3551165e6c49a1bb32f7bdbe8e9a98f9e90229bb7071ca2b5d28ce2db34'),
        (11, 62, 0, (14909440.0, 8945664.0), 492011520.0, '7d9e820aecf0f5991f19c18b72d9ecdbca57aee8a812d87b250620cbd5b7ebe0'),
        (21, 93, 0, (17203200.0, 10059776.0), 567705600.0, 'a2e91d7b6c699cdd61f02bbf43f9d53a0b7578c0785bd11f11b7ab4b2879739e'),
    ),
    'resident 104, 32: fusion 2 scope 0 overlap 1 hand-over 0': (
        (20, 31, 0, (17203200.0, 8568832.0), 567705600.0, 'f117a3551165e6c49a1bb32f7bdbe8e9a98f9e90229bb7071ca2b5d28ce2db34'),
        (11, 62, 0, (14909440.0, 8945664.0), 492011520.0, '7d9e820aecf0f5991f19c18b72d9ecdbca57aee8a812d87b250620cbd5b7ebe0'),
        (21, 93, 0, (17203200.0, 8568832.0), 567705600.0, 'a2e91d7b6c699cdd61f02bbf43f9d53a0b7578c0785bd11f11b7ab4b2879739e'),
    ),
    'resident 104, 32: fusion 2 scope 0 overlap 0 hand-over 0': (
        (20, 31, 0, (17203200.0, 8601600.0), 567705600.0, '17b1b056086f50f40e179f60a2ba34183fe16f2b6114346be05cda7f835ed6b7'),
        (11, 62, 0, (14909440.0, 8945664.0), 492011520.0, '481c9713120ebaee141f85dd50010c220acf125e6d250c07f91f3de6b94c74c8'),
        (21, 93, 0, (17203200.0, 8601600.0), 567705600.0, 'a59c4135d0365d479256e2c217c46a1d369e6b80a521d34453cb237def7ddac4'),
    ),
    'resident 104, 32: fusion 2 scope 1 overlap 1 hand-over 1': (
        (20, 31, 0, (17203200.0, 10059776.0), 567705600.0, 'f117a3551165e6c49a1bb32f7bdbe8e9a98f9e90229bb7071ca2b5d28ce2db34'),
        (21, 62, 31, (17203200.0, 8568832.0), 567705600.0, '3dfe6a2779bb3f22ad00af2d8c41fe8e2a26792e924ce3525440bd58e336b22c'),
        (21, 93, 62, (17203200.0, 8568832.0), 567705600.0, 'eb902fca7590ad96b52fd5dcad44a14ad19354b56249260c5b88cd66d3603987'),
    ),
    'resident 104, 32: fusion 2 scope 1 overlap 1 hand-over 0': (
        (20, 31, 0, (17203200.0, 8568832.0), 567705600.0, 'f117a3551165e6c49a1bb32f7bdbe8e9a98f9e90229bb7071ca2b5d28ce2db34'),
        (21, 62, 0, (17203200.0, 8568832.0), 567705600.0, 'bd1d1537a66bdb804f717b6262a05bdfb5c26b74c45dbebeab13b031440be6a6'),
        (21, 93, 0, (17203200.0, 8568832.0), 567705600.0, '1b533bd4292bf8c093ee567da22fd29ae08e761c97be1f0124225367e7aae1c8'),
    ),
    'resident 104, 32: fusion 2 scope 1 overlap 0 hand-over 0': (
        (20, 31, 0, (17203200.0, 8601600.0), 567705600.0, '17b1b056086f50f40e179f60a2ba34183fe16f2b6114346be05cda7f835ed6b7'),
        (21, 62, 0, (17203200.0, 8601600.0), 567705600.0, 'd3923d0f09b2137fb7b346471b108880035c51d8ce65c335c55104a67888d2f6'),
        (21, 93, 0, (17203200.0, 8601600.0), 567705600.0, 'b7f6943e003dcbecf416cdd19767f6cc848c8aa19d5fc9bc4b0081a8a2ad57e9'),
    ),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c['name'] for c in CASES])
def test_a_launch_is_what_it_was_before_the_plan(name):
    got = measure(BY_NAME[name])
    want = BEFORE[name]
    for k, (g, w) in enumerate(zip(got, want)):
        print("%s, step %d: %r" % (name, k, g))
        assert g[0] == TRACES[w[0]], (k, g[0], TRACES[w[0]])
        assert g[1:] == w[1:], (k, g[1:], w[1:])
    assert len(got) == len(want)


@pytest.mark.gpu
def test_every_instantiation_is_among_the_cases():
    """The eight kernels, by the names the launch trace gives them."""
    seen = {name for t in TRACES for name, _n in t if 'prop_fused_kernel' in name}
    assert seen == {'(prop_fused_kernel<true, 6>)', '(prop_fused_kernel<true, 0>)', '(prop_fused_kernel<false, 7>)',
                    '(prop_fused_kernel<false, 6>)', '(prop_fused_kernel<false, 5>)', '(prop_fused_kernel<false, 0>)',
                    '(prop_fused_kernel<false, 7, true, true>)', '(prop_fused_kernel<false, 7, true, false>)'}, seen
