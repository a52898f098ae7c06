"""Gamma, loggamma, digamma and trigamma on the device (pytest -m gpu).

Models (tools/problems.py): ``mathfn_e`` -- one or two functions of csrc/sa_math_gamma.h per output (loggamma / gamma /
digamma / factorial; trigamma through the derivative of digamma), a state times or over a differentiated parameter as
the argument; ``gamma_delay`` -- a gamma-density forcing with an inferred shape and loggamma / gamma / digamma terms of
the states in one integrated right-hand side (callbacks pinned by hand-written closed forms and the truth fixture,
tests/test_gamma_math.py).

Bars: device == oracle BIT FOR BIT (statuses, counters, every fp64 output) -- the generated header embeds
csrc/sa_math.h and csrc/sa_math_gamma.h, so host and device execute one IEEE operation sequence; device vs DOP853 truth
at the bars of tests/test_gpu_transcendental.py (states <= 1e-5, gradients <= 4e-6 relative at rtol = atol = 1e-8).
"""
import numpy as np
import pytest

from tests import family_checks as fc
from tools.family_models import FAMILY

pytestmark = pytest.mark.gpu

#: device vs truth: the bars of tests/test_gpu_transcendental.py
BARS = dict(y=1e-5, grad=4e-6)


def _points(N):
    """States and parameters of ``mathfn_e`` that put the arguments into EVERY piece of every function (the boundaries:
    codegen.math_boundaries("gamma")), onto the negative axis (a negative parameter) and, for one point in 32, exactly
    onto a pole (a = 1 and a non-positive integer state) or beyond the overflow of Gamma."""
    rng = np.random.RandomState(11)

    def sign(p_neg=0.35):
        return rng.choice([-1.0, 1.0], N, p=[p_neg, 1.0 - p_neg])
    y = np.stack([10.0 ** rng.uniform(-2.5, 1.4, N),            # loggamma(a x): 0.002 .. 50, all pieces below 1e17
                  rng.uniform(0, 12, N),                        # gamma(x / a): every stage of the recurrence
                  10.0 ** rng.uniform(-2, 1.5, N),              # digamma(a x), trigamma(a x): 0.005 .. 60
                  10.0 ** rng.uniform(-2, 1.3, N),              # loggamma(a x) + digamma(x / a)
                  rng.uniform(0, 8, N)], axis=1)                # factorial(a x) = gamma(1 + a x)
    par = np.stack([rng.uniform(0.5, 2, N) * sign(), rng.uniform(0.5, 2, N) * sign(), rng.uniform(0.5, 2, N) * sign(),
                    rng.uniform(0.5, 2, N) * sign(), rng.uniform(0.3, 1.5, N) * sign()], axis=1)
    y[0::64, 0] = 10.0 ** rng.uniform(17.1, 19, len(y[0::64]))  # lgamma's last piece, x (ln x - 1)
    pole = np.arange(N) % 32 == 5
    par[pole] = 1.0
    y[pole] = -rng.randint(0, 6, (int(pole.sum()), 5)).astype(float)
    y[pole, 4] -= 1.0                                           # 1 + a x = 0, -1, ...
    over = np.arange(N) % 32 == 21
    y[over, 1] = rng.uniform(172, 400, int(over.sum()))
    par[over, 1] = 1.0
    return y, par, rng.randn(N, 5), rng.uniform(0, 50, N)


def test_points_reach_every_piece_the_negative_axis_and_the_poles():
    """(no device work: what the bitwise comparison below is made on)"""
    from sunode_amd.symode import codegen
    y, par, _, _ = _points(4096)
    bounds = codegen.math_boundaries("gamma")
    args = {"lgamma": np.concatenate([par[:, 0] * y[:, 0], par[:, 3] * y[:, 3]]),
            "tgamma": np.concatenate([y[:, 1] / par[:, 1], 1 + par[:, 4] * y[:, 4]]),
            "digamma": np.concatenate([par[:, 2] * y[:, 2], y[:, 3] / par[:, 3]]),
            "trigamma": np.concatenate([par[:, 2] * y[:, 2], y[:, 3] / par[:, 3]])}
    for fn, u in args.items():
        pos = u[u > 0]
        pieces = np.bincount(np.searchsorted(np.array(bounds[fn]), pos, side="right"), minlength=len(bounds[fn]) + 1)
        assert (pieces >= 8).all(), (fn, pieces)
        assert (u < 0).sum() >= 400 and ((u <= 0) & (u == np.round(u))).sum() >= 32, fn


def test_device_gamma_library_equals_host_bitwise():
    """4 096 points through the generated callbacks of ``mathfn_e``: all five callbacks and the return codes are the
    host's, bit for bit (two NaNs count as equal -- and at least 60 % of the points of every output are finite in the
    oracle, so NaN == NaN cannot carry the comparison)."""
    fc.callbacks_equal_host_bitwise("mathfn_e", *_points(4096))     # (not finite: on a pole or beyond the overflow)


def test_gamma_delay_forward_adjoint_bitexact_vs_oracle():
    """B = 300 (four full wavefronts and a ragged one): statuses, step / order counters and every output equal the
    oracle's bit for bit, through AdjointSolver and the plain Solver."""
    fc.forward_adjoint_bitexact("gamma_delay", 300)


@pytest.mark.parametrize("group", FAMILY["gamma_delay"].mappings)
def test_gamma_delay_through_the_other_mappings(group, monkeypatch):
    """The callbacks staged through LDS (4-lane groups), run by a 4-wavefront workgroup and out of the HBM workspace:
    still the oracle's bits (B = 70)."""
    fc.through_mapping("gamma_delay", 70, group, monkeypatch)


def test_gamma_delay_forward_sensitivities():
    """``Solver(sens_mode="simultaneous")`` at B = 64 (5 differentiated parameters x 3 states): states and
    sensitivities equal the oracle's bit for bit."""
    fc.forward_sens_bitexact("gamma_delay", 64, "simultaneous")


def test_gamma_delay_matches_truth(golden_dir):
    """Device vs DOP853 truth (tests/golden/truth_gamma_delay.npz, 16 draws): states <= 1e-5, gradients and -lamda
    <= 4e-6 relative to the per-draw maximum."""
    fc.matches_truth("gamma_delay", golden_dir, BARS)


def test_reaching_the_pole_is_a_per_instance_failure():
    """b = 6 on one draw of 64 drives 1 - b x into the pole of Gamma at 0 (a finite-time blow-up of x): that instance
    reports the oracle's failure status with NaN outputs -- an ordinary solver status --, the other 63 equal the oracle
    bit for bit."""
    fc.per_instance_failure("gamma_delay", 5, 2, 6.0)
