"""erfinv, erfcinv and the incomplete gamma functions on the device (pytest -m gpu).

Models (tools/problems.py): ``mathfn_g`` -- one or two functions of csrc/sa_math_prob.h per output, the time as the
run-time shape of the incomplete gamma functions; ``quantile_delay`` -- a gamma-delay CDF (lowergamma), a probit
transform of a state (erfinv) and a survival function (uppergamma) in one integrated right-hand side (callbacks pinned
by hand-written closed forms and the truth fixture, tests/test_prob_math.py).

Bars: device == oracle BIT FOR BIT (statuses, counters, every fp64 output) -- the generated header embeds
csrc/sa_math.h, sa_math_inv.h, sa_math_gamma.h and sa_math_prob.h, so host and device execute one IEEE operation
sequence, the run-time trip counts of the series and of the continued fraction included; device vs DOP853 truth at the
bars of the gamma family (states <= 1e-5, gradients <= 4e-6 relative at rtol = atol = 1e-8).
"""
import pytest

from tests import family_checks as fc
from tools.family_models import FAMILY
from tools.problems import mathfn_g_points

pytestmark = pytest.mark.gpu

#: device vs truth: the bars of tests/test_gpu_gamma.py
BARS = dict(y=1e-5, grad=4e-6)


def test_device_prob_library_equals_host_bitwise():
    """4 096 points through the generated callbacks of ``mathfn_g`` -- three quarters inside every function's domain, in
    every piece and on every boundary constant; the rest outside (|u| > 1, a shape above 32, a negative argument) --:
    all five callbacks and the return codes are the host's, bit for bit (at least 60 % of the points of every output are
    finite in the oracle: tests/test_prob_math.py checks the share without a device)."""
    fc.callbacks_equal_host_bitwise("mathfn_g", *mathfn_g_points(4096))


def test_quantile_delay_forward_adjoint_bitexact_vs_oracle():
    """B = 64: statuses, step / order counters and every output equal the oracle's bit for bit, through AdjointSolver and
    the plain Solver."""
    fc.forward_adjoint_bitexact("quantile_delay", 64)


@pytest.mark.parametrize("group", FAMILY["quantile_delay"].mappings)
def test_quantile_delay_through_the_other_mappings(group, monkeypatch):
    """The callbacks staged through LDS (4-lane groups), run by a 4-wavefront workgroup and out of the HBM workspace:
    still the oracle's bits (B = 64)."""
    fc.through_mapping("quantile_delay", 64, group, monkeypatch)


@pytest.mark.parametrize("mode", ["simultaneous", "staggered"])
def test_quantile_delay_forward_sensitivities(mode):
    """``Solver(sens_mode=mode)`` at B = 64 (5 differentiated parameters x 3 states), both correctors: states and
    sensitivities equal the oracle's bit for bit."""
    fc.forward_sens_bitexact("quantile_delay", 64, mode)


def test_quantile_delay_matches_truth(golden_dir):
    """Device vs DOP853 truth (tests/golden/truth_quantile_delay.npz, 16 draws): states <= 1e-5, gradients and -lamda
    <= 4e-6 relative to the per-draw maximum."""
    fc.matches_truth("quantile_delay", golden_dir, BARS)


def test_leaving_the_domain_of_erfinv_is_a_per_instance_failure():
    """b = 6 on one draw of 64 puts b (2 x - 1) beyond -1, outside erfinv's domain: that instance reports the oracle's
    failure status with NaN outputs -- an ordinary solver status --, the other 63 equal the oracle bit for bit."""
    fc.per_instance_failure("quantile_delay", 5, 1, 6.0)
