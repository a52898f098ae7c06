"""Bessel functions J, Y, I, K of integer order on the device (pytest -m gpu).

Models (tools/problems.py): ``mathfn_f`` -- one or two functions of csrc/sa_math_bessel.h per output (besselj /
bessely / besseli / besselk; further orders through the derivatives), a state times or over a differentiated parameter
as the argument; ``bessel_ring`` -- an I1 / I0 drive of a state, a J0 forcing with an inferred wavenumber, a K0 source,
a Y1 push and a Y0 read-out in one integrated right-hand side (callbacks pinned by hand-written closed forms and the truth
fixture, tests/test_bessel_math.py).

Bars: device == oracle BIT FOR BIT (statuses, counters, every fp64 output) -- the generated header embeds
csrc/sa_math.h and csrc/sa_math_bessel.h, so host and device execute one IEEE operation sequence; device vs DOP853
truth at the bars of tests/test_gpu_transcendental.py (states <= 1e-5, gradients <= 4e-6 relative at rtol = atol = 1e-8).
"""
import numpy as np
import pytest

from tests import family_checks as fc
from tests.helpers import make_oracle
from tools.family_models import FAMILY

pytestmark = pytest.mark.gpu

#: device vs truth: the bars of tests/test_gpu_transcendental.py
BARS = dict(y=1e-5, grad=4e-6)
#: the draw of 64 whose g is raised, and the value: z reaches 1 + x and the argument of Y1 and Y0 goes through zero
FAIL_DRAW, FAIL_G = 5, 6.0


def _points(N):
    """States and parameters of ``mathfn_f`` that put the arguments into EVERY piece of every function (the boundaries:
    codegen.math_boundaries("bessel")), onto the negative axis (a negative parameter), for one point in 32 exactly
    onto zero, beyond the domain of J (2^50), beyond I's overflow and beyond K's underflow."""
    rng = np.random.RandomState(11)

    def sign(p_neg):
        return rng.choice([-1.0, 1.0], N, p=[p_neg, 1.0 - p_neg])
    y = np.stack([10.0 ** rng.uniform(-2, 1.7, N),              # J0(a x), J1: 0.005 .. 100
                  10.0 ** rng.uniform(-2, 1.7, N),              # Y1(x / a), Y0, Y2
                  10.0 ** rng.uniform(-1, 2.95, N),             # I2(a x), I1, I3: 0.05 .. 1 780, +inf beyond 714
                  10.0 ** rng.uniform(-2.5, 1.6, N),            # K0(a x) + J2(x / a): 0.0015 .. 80
                  10.0 ** rng.uniform(-2, 2.95, N)], axis=1)    # K1(x / a), K0, K2: +0 beyond 745
    par = np.stack([rng.uniform(0.5, 2, N) * sign(0.35), rng.uniform(0.5, 2, N) * sign(0.15), rng.uniform(0.5, 2, N) * sign(0.35),
                    rng.uniform(0.5, 2, N) * sign(0.15), rng.uniform(0.5, 2, N) * sign(0.15)], axis=1)
    y[np.arange(N) % 32 == 5] = 0.0                             # J0 = 1, I2 = 0, Y1 = -inf, K = +inf
    far = np.arange(N) % 32 == 21
    y[far, 0] = 10.0 ** rng.uniform(15.5, 18, int(far.sum()))   # beyond 2^50: NaN
    return y, par, rng.randn(N, 5), rng.uniform(0, 50, N)


def _arguments(y, par):
    return {"j": par[:, 0] * y[:, 0], "y": y[:, 1] / par[:, 1], "i": par[:, 2] * y[:, 2], "k0": par[:, 3] * y[:, 3],
            "jn": y[:, 3] / par[:, 3], "k1": y[:, 4] / par[:, 4]}


def test_points_reach_every_piece_the_negative_axis_zero_and_the_range_limits():
    """(no device work: what the bitwise comparison below is made on)"""
    from sunode_amd.symode import codegen
    y, par, lam, t = _points(4096)
    bounds = codegen.math_boundaries("bessel")
    u = _arguments(y, par)
    use = {"j0": u["j"], "j1": u["j"], "y0": u["y"], "y1": u["y"], "i0": u["i"], "i1": u["i"], "in": u["i"],
           "k0": u["k0"], "k1": u["k1"], "jn": u["jn"]}
    assert set(use) == set(bounds)
    for fn, arg in use.items():
        bs = list(bounds[fn]) + ([2.0] if fn == "jn" else [])      # J2: downwards below |x| = 2, upwards from there on
        a = np.abs(arg[arg != 0]) if fn[0] in "ji" else arg[arg > 0]
        pieces = np.bincount(np.searchsorted(np.array(sorted(bs)), a, side="right"), minlength=len(bs) + 1)
        assert (pieces >= 8).all(), (fn, pieces)
    for key, arg in u.items():
        assert (arg < 0).sum() >= 400 and (arg == 0).sum() >= 100, key
    assert (np.abs(u["j"]) > 2.0 ** 50).sum() >= 100
    assert (np.abs(u["i"]) > 714).sum() >= 8 and (u["k1"] > 746).sum() >= 8
    # the condition of the bitwise test, met by the oracle alone: at least 60 % of every output finite, some not
    orc = make_oracle("mathfn_f")
    keys = ("rhs", "jac", "adj", "quad", "adjjac")
    finite = {key: 0 for key in keys}
    N = len(y)
    for i in range(N):
        host = orc.eval(t[i], y[i], lam[i], par[i], np.zeros(0))
        for key in keys:
            finite[key] = finite[key] + np.isfinite(np.asarray(host[key]).ravel())
    for key in keys:
        assert (finite[key] >= 0.6 * N).all(), (key, finite[key] / N)
        assert (finite[key] < N).any(), key
    assert (finite["rhs"] < N).all()                  # some points of EVERY output are non-finite


def test_device_bessel_library_equals_host_bitwise():
    """4 096 points through the generated callbacks of ``mathfn_f``: all five callbacks and the return codes are the
    host's, bit for bit (two NaNs count as equal -- and at least 60 % of the points of every output are finite in the
    oracle, so NaN == NaN cannot carry the comparison)."""
    fc.callbacks_equal_host_bitwise("mathfn_f", *_points(4096))     # (not finite: zero, negative or beyond a range limit)


def test_bessel_ring_forward_adjoint_bitexact_vs_oracle():
    """B = 300 (four full wavefronts and a ragged one): statuses, step / order counters and every output equal the
    oracle's bit for bit, through AdjointSolver and the plain Solver."""
    fc.forward_adjoint_bitexact("bessel_ring", 300)


@pytest.mark.parametrize("group", FAMILY["bessel_ring"].mappings)
def test_bessel_ring_through_the_other_mappings(group, monkeypatch):
    """The callbacks staged through LDS (4-lane groups), run by a 4-wavefront workgroup and out of the HBM workspace:
    still the oracle's bits (B = 70)."""
    fc.through_mapping("bessel_ring", 70, group, monkeypatch)


def test_bessel_ring_forward_sensitivities():
    """``Solver(sens_mode="simultaneous")`` at B = 64 (5 differentiated parameters x 3 states): states and
    sensitivities equal the oracle's bit for bit."""
    fc.forward_sens_bitexact("bessel_ring", 64, "simultaneous")


def test_bessel_ring_matches_truth(golden_dir):
    """Device vs DOP853 truth (tests/golden/truth_bessel_ring.npz, 16 draws): states <= 1e-5, gradients and -lamda
    <= 4e-6 relative to the per-draw maximum."""
    fc.matches_truth("bessel_ring", golden_dir, BARS)


def test_an_argument_of_y0_through_zero_is_a_per_instance_failure():
    """g = 6 on one draw of 64 lets z approach 1 + x; -r Y1(1 + x - z) then drives the argument of Y1 and Y0 through
    zero in finite time (-inf there, NaN beyond): that instance reports the oracle's failure status with NaN outputs -- an ordinary solver
    status --, the other 63 equal the oracle bit for bit."""
    fc.per_instance_failure("bessel_ring", FAIL_DRAW, 2, FAIL_G)
