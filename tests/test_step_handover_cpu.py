"""The re-association behind the step hand-over (afq_set_step_handover), on the reference alone: the next step's opening pass
is made as (B B) S -- B B rounded once from an extended-precision product on the host, S the Taylor sum -- where the step itself
would make B (B S).  For the three shapes of tests.test_gpu_step_handover and their one-body matrices, both forms in double
precision are held to the product in numpy.longdouble: the error of either, and their difference, relative to the largest
element, stay below TOL / 100 -- the device tolerance of 1e-10 per step is not what hides the re-association.  The measured
values are recorded in profiles/step_handover_precision.md."""
import numpy
import pytest

from tests.test_gpu_sizes import build

K = 8
SHAPES = [(97, 17), (100, 25), (104, 32)]
TOL = 1e-10


def reassociation_errors(M, N):
    model, rng = build(M, K, N, N, False, seed=31, dt=0.01)
    B = numpy.ascontiguousarray(model.BH1[0].real)
    assert numpy.abs(model.BH1.imag).max() == 0.0
    S = model.psi[:, :N] + 0.1 * (rng.rand(M, N) + 1j * rng.rand(M, N))
    Bl, Sl = B.astype(numpy.longdouble), S.astype(numpy.clongdouble)
    exact = Bl.dot(Bl.dot(Sl))
    B2 = Bl.dot(Bl).astype(numpy.float64)                       # the host's B B: extended accumulation, one rounding
    handed = B2.dot(S)
    plain = B.dot(B.dot(S))
    scale = float(numpy.abs(exact).max())
    return (float(numpy.abs(handed - exact).max()) / scale, float(numpy.abs(plain - exact).max()) / scale,
            float(numpy.abs(handed - plain).max()) / scale)


@pytest.mark.parametrize("M,N", SHAPES)
def test_b_squared_times_s_is_b_times_b_s_far_below_the_device_tolerance(M, N):
    assert numpy.finfo(numpy.longdouble).eps < 1e-18            # an extended reference, not double under another name
    handed, plain, apart = reassociation_errors(M, N)
    print("M=%d n=%d  (B B) S: %.3e  B (B S): %.3e  difference: %.3e" % (M, N, handed, plain, apart))
    assert handed < TOL / 100.0, handed
    assert plain < TOL / 100.0, plain
    assert apart < TOL / 100.0, apart
