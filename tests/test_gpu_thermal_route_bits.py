"""The routes of the thermal walkers that the recorded paths of tests/test_gpu_thermal_hubbard_cont.py do not reach --
the wide engine with complex and with real matrices (thermal_wide.h), the delayed slice (thermal_slice_delayed_kernel)
and the two wide slice kernels -- held to recorded bits: SHA-256 over the arrays' bytes, two walkers each, a few
seconds a case.  The other tests of these routes hold them to tolerances and to each other; these hold them to what
they computed before the engines were given one kernel per arithmetic."""
import os

import numpy
import pytest

from pauxy_amd import _lib as L
from tests import thermal_delayed_cases as D
from tests.test_gpu_thermal_hubbard_cont import digest, hubbard_continuous_digest, ueg_path_digest
from tests.test_gpu_thermal_wide import chain, complex_stack
from tests.thermal_cases import Case

pytestmark = pytest.mark.gpu

WIDE = L.THERMAL_WIDE
HERE = os.path.dirname(os.path.abspath(__file__))


def wide_greens_digest(M):
    """G and det of the complex wide engine on uploaded bins of a Hubbard chain: 2 walkers, 3 bins of 2 slices, at
    slice_ix 0 (the chain starts at bin 1) and 3 (at bin 2)."""
    stack = complex_stack(M, 2, 3, 2, 5)
    dev = chain(M, 6).device(2, 2, WIDE)
    try:
        dev.set(L.F_THERMAL_STACK, stack)
        out = []
        for s in (0, 3):
            dev.thermal_greens(s)
            out += [dev.get(L.F_THERMAL_G), dev.get(L.F_THERMAL_DET)]
        return digest(out)
    finally:
        dev.close()


def delayed_path_digest(case, us, Lts, stack_size, nstblz):
    """A two-walker path on a delayed handle: the fields chosen, G, the bins and the weights behind every slice."""
    dev = D.delayed_device(case, 2, Lts, stack_size, nstblz)
    try:
        out = [dev.get(L.F_THERMAL_G)]                               # the trial's, by the wide real engine
        for u in us:
            out.append(dev.thermal_propagate(u, 0.0, fetch_fields=True))
            out += [dev.get(L.F_THERMAL_G), dev.get(L.F_THERMAL_STACK), dev.get(L.F_WEIGHT)]
        return digest(out)
    finally:
        dev.close()


def delayed_65_digest():
    """5 x 13 of thermal_hubbard_large.npz (case c: stack_size 5, nstblz 5), the fixture's uniforms for walker 0 and a
    stream of RandomState(42) for walker 1, 6 slices: slice 5 rebuilds G from the bins, every slice wraps.  M = 65 is
    the first M beyond one lane per column, and the last panel of the delayed slice holds one site."""
    d = numpy.load(os.path.join(HERE, "golden", "thermal_hubbard_large.npz"))
    c = D.FixtureCase(d, 'c')
    rng = numpy.random.RandomState(42)
    us = [numpy.array([d['c_u'][ts], rng.random_sample(c.M)]) for ts in range(6)]
    return delayed_path_digest(c, us, c.L, c.stack_size, c.nstblz)


def delayed_16_digest():
    """4 x 4: a single panel of the delayed slice, a single MFMA tile of the wide real engine; stack_size 2 and nstblz
    2 over 4 slices (both branches of the in-bin counter, two rebuilds)."""
    case = Case(4, 4, 4.0, 0.05, mu=1.0, mu_trial=0.8)
    us = numpy.random.RandomState(16).random_sample((4, 2, case.M))
    return delayed_path_digest(case, us, 4, 2, 2)


# recorded by running the functions above on an MI355X with the library of the commit before the thermal engines were
# merged into one kernel per arithmetic (the parent of the commit that added this file)
BITS_BEFORE = {
    'complex wide Green 19': "b427a977f574764350b31baaf2f87bd41cf42f25ea10bfcd03f44ce6c3b4cd3f",
    'complex wide Green 81': "a83bd0811f1df53ea53c8343e3f877439120ea6308cf00974d0c37e0dce19b07",
    'delayed 5x13': "9a13ca20b21115d9c1ba3b5b999fe0bedadd7b2a8ee631340d240d5a37b75506",
    'delayed 4x4': "efd917014696833607d1c412b29f05635dd98ee50778e54243aa270741617ed8",
    'ueg a2_ wide': ("bee62725cd497a11a401d032b70b415d1e8a5c9ae80ad2d8d08b80b55f378012", 0),
    'hubbard a0_ wide': ("e3e7df01d0dd39f589a6e9b436edd56798abf4ca479626d3b59c5435e1b9fa26", 0),
}

CASES = {
    'complex wide Green 19': lambda: wide_greens_digest(19),        # one full and one ragged 16-tile
    'complex wide Green 81': lambda: wide_greens_digest(81),        # a lane owns a second column (c + 64)
    'delayed 5x13': delayed_65_digest,
    'delayed 4x4': delayed_16_digest,
    'ueg a2_ wide': lambda: ueg_path_digest('a2_', WIDE, with_count=True),          # (digest, counters()[0])
    'hubbard a0_ wide': lambda: hubbard_continuous_digest('a0_', WIDE),
}


@pytest.mark.parametrize("key", sorted(BITS_BEFORE), ids=lambda k: k.replace(" ", "_"))
def test_wide_and_delayed_routes_keep_their_bits(key):
    got = CASES[key]()
    print("%r: %r," % (key, got))
    assert got == BITS_BEFORE[key]
