"""Inverse trigonometric / inverse hyperbolic functions and erf / erfc on the device (pytest -m gpu).

Models (tools/problems.py): ``mathfn_c`` (asin / acos / atan / atan2) and ``mathfn_d`` (asinh / acosh / atanh / erf /
erfc) -- one or two functions of csrc/sa_math_inv.h per output, a state times or over a differentiated parameter as
the argument; ``probit_gate`` -- all nine in one integrated right-hand side (callbacks pinned by hand-written closed
forms and the truth fixture, tests/test_inverse_erf_math.py).

Bars: device == oracle BIT FOR BIT (statuses, counters, every fp64 output) -- the generated header embeds
csrc/sa_math.h and csrc/sa_math_inv.h, so host and device execute one IEEE operation sequence; device vs DOP853 truth
at the bars of tests/test_gpu_transcendental.py (states <= 1e-5, gradients <= 4e-6 relative at rtol = atol = 1e-8).
"""
import numpy as np
import pytest

from tests import family_checks as fc
from tools.family_models import FAMILY

pytestmark = pytest.mark.gpu

#: device vs truth: the bars of tests/test_gpu_transcendental.py
BARS = dict(y=1e-5, grad=4e-6)


def _points(name, N):
    """States and parameters that put the arguments into EVERY interval of every function (the boundaries:
    codegen.math_boundaries("inv")) and, for a minority of the points, outside the domains."""
    rng = np.random.RandomState(7)

    def sign(p_neg=0.5):
        return rng.choice([-1.0, 1.0], N, p=[p_neg, 1.0 - p_neg])
    if name == "mathfn_c":
        y = np.stack([rng.uniform(0, 1.15, N),                  # asin(a x): |a x| up to 1.2
                      rng.uniform(0, 1.1, N),                   # acos(x / a): up to 1.4
                      np.exp(rng.uniform(-6, 4, N)),            # atan(a x): e^-9 .. e^6, all five intervals
                      np.exp(rng.uniform(-6, 4, N)) * sign(),   # atan2(x, a): four quadrants
                      rng.uniform(0, 3, N)], axis=1)            # atan2(a, x - 2) + asin(x / a)
        par = np.stack([rng.uniform(0.3, 1.05, N) * sign(), rng.uniform(0.8, 3, N) * sign(),
                        np.exp(rng.uniform(-3, 2, N)) * sign(), np.exp(rng.uniform(-3, 2, N)) * sign(),
                        rng.uniform(1, 4, N) * sign()], axis=1)
    else:
        y = np.stack([10.0 ** rng.uniform(-10, 155, N),         # asinh(a x): 1e-13 .. 1e158, across 2^500
                      10.0 ** rng.uniform(-10, 155, N),         # acosh(1 + a x): across 2^500; a < 0: below 1
                      rng.uniform(0, 1.1, N),                   # atanh(x / a): both sides of 1/2, beyond 1
                      rng.uniform(0, 6, N),                     # erf(a x): |a x| up to 30, all six pieces
                      rng.uniform(0, 27, N)], axis=1)           # erfc(x / a): -34 .. 34
        par = np.stack([10.0 ** rng.uniform(-3, 3, N) * sign(), 10.0 ** rng.uniform(-3, 3, N) * sign(0.2),
                        rng.uniform(0.3, 3, N) * sign(), rng.uniform(0.01, 5, N) * sign(),
                        rng.uniform(0.8, 2, N) * sign()], axis=1)
    return y, par, rng.randn(N, 5), rng.uniform(0, 50, N)


@pytest.mark.parametrize("name", ["mathfn_c", "mathfn_d"])
def test_device_inverse_erf_library_equals_host_bitwise(name):
    """4 096 points through the generated callbacks whose outputs are single functions of sa_math_inv.h and their
    derivatives: all five callbacks and the return codes are the host's, bit for bit (two NaNs count as equal -- and
    at least 60 % of the points of every output are finite in the oracle, so NaN == NaN cannot carry the comparison)."""
    fc.callbacks_equal_host_bitwise(name, *_points(name, 4096))     # (not finite: outside a domain)


def test_probit_gate_forward_adjoint_bitexact_vs_oracle():
    """B = 300 (four full wavefronts and a ragged one): statuses, step / order counters and every output equal the
    oracle's bit for bit, through AdjointSolver and the plain Solver."""
    fc.forward_adjoint_bitexact("probit_gate", 300)


@pytest.mark.parametrize("group", FAMILY["probit_gate"].mappings)
def test_probit_gate_through_the_other_mappings(group, monkeypatch):
    """The callbacks staged through LDS (4-lane groups), run by a 4-wavefront workgroup and out of the HBM workspace:
    still the oracle's bits (B = 70)."""
    fc.through_mapping("probit_gate", 70, group, monkeypatch)


def test_probit_gate_forward_sensitivities():
    """``Solver(sens_mode="simultaneous")`` at B = 64 (5 differentiated parameters x 3 states): states and
    sensitivities equal the oracle's bit for bit."""
    fc.forward_sens_bitexact("probit_gate", 64, "simultaneous")


def test_probit_gate_matches_truth(golden_dir):
    """Device vs DOP853 truth (tests/golden/truth_probit_gate.npz, 16 draws): states <= 1e-5, gradients and -lamda
    <= 4e-6 relative to the per-draw maximum."""
    fc.matches_truth("probit_gate", golden_dir, BARS)


def test_out_of_domain_argument_is_a_per_instance_failure():
    """b = 4 on one draw of 64 drives asin(b x / (1 + z)) beyond 1: that instance reports the oracle's failure status
    with NaN outputs -- an ordinary solver status --, the other 63 equal the oracle bit for bit."""
    fc.per_instance_failure("probit_gate", 5, 4, 4.0)
