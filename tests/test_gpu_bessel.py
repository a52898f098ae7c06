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
import functools
import os

import numpy as np
import pytest

from tests.helpers import make_oracle, make_problem
from tools.problems import bessel_ring_batch

pytestmark = pytest.mark.gpu

CMP = [0, 1, 2, 3, 4, 5, 6, 7, 8]
CMP_B = [0, 1, 2, 3, 4, 5, 6, 9, 10, 12]
TOL = dict(abstol=1e-8, reltol=1e-8, backward_abstol=1e-8, backward_reltol=1e-8, quad_abstol=1e-8, quad_reltol=1e-8)
#: the draw of 64 whose g is raised, and the value: z reaches 1 + x and the argument of Y1 and Y0 goes through zero
FAIL_DRAW, FAIL_G = 5, 6.0


@functools.lru_cache(maxsize=None)
def _oracle_run(B):
    """Forward + adjoint of the B-draw batch of ``bessel_ring`` in the oracle (computed once per batch size)."""
    d = bessel_ring_batch(B)
    orc = make_oracle("bessel_ring")
    cfg = orc.config(rtol=1e-8, atol=1e-8, rtolB=1e-8, atolB=1e-8, rtolQB=1e-8, atolQB=1e-8)
    tv = d["tvals"]
    fwd = orc.solve_forward(cfg, d["y0"], d["ps"], d["pr"], 0.0, tv, nthreads=8)
    bwd = orc.solve_backward(cfg, tv[-1], 0.0, tv, d["grads"], nthreads=8)
    return d, fwd, bwd


def _points(N):
    """States and parameters of ``mathfn_f`` that put the arguments into EVERY piece of every function (the boundaries:
    codegen.math_bessel_boundaries()), onto the negative axis (a negative parameter), for one point in 32 exactly
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
    bounds = codegen.math_bessel_boundaries()
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
    from sunode_amd.solver import Solver
    prob = make_problem("mathfn_f")
    eng = Solver(prob)._engine()
    orc = make_oracle("mathfn_f")
    N = 4096
    y, par, lam, t = _points(N)
    with np.errstate(all="ignore"):
        got = eng.eval_callbacks(t, y, lam, par, np.zeros((N, 0)))
    keys = ("rhs", "jac", "adj", "quad", "adjjac")
    differing = 0
    finite = {key: 0 for key in keys}
    for i in range(N):
        host = orc.eval(t[i], y[i], lam[i], par[i], np.zeros(0))
        for key in keys:
            a, b = np.asarray(got[key][i]).ravel(), np.asarray(host[key]).ravel()
            differing += int(np.sum((a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))))
            finite[key] = finite[key] + np.isfinite(b)
        assert got["codes"][i].tolist() == np.asarray(host["codes"]).tolist()
    assert differing == 0
    for key in keys:
        assert (finite[key] >= 0.6 * N).all(), (key, finite[key] / N)
        assert (finite[key] < N).any(), key           # (and some arguments were zero, negative or beyond a range limit)


def test_bessel_ring_forward_adjoint_bitexact_vs_oracle():
    """B = 300 (four full wavefronts and a ragged one): statuses, step / order counters and every output equal the
    oracle's bit for bit, through AdjointSolver and the plain Solver."""
    from sunode_amd.solver import AdjointSolver, Solver
    prob = make_problem("bessel_ring")
    d, (yo, so, sto), (go, lo, sbo, stbo) = _oracle_run(300)
    tv = d["tvals"]
    sol = AdjointSolver(prob, **TOL)
    y, st, stats = sol.solve_forward_batch(0.0, tv, d["y0"], d["ps"], d["pr"])
    g, lam, stb, statsb = sol.solve_backward_batch(tv[-1], 0.0, tv, d["grads"])
    assert (st == 0).all() and (stb == 0).all() and (so == 0).all() and (sbo == 0).all()
    np.testing.assert_array_equal(stats[:, CMP], sto[:, CMP])
    np.testing.assert_array_equal(y, yo)
    np.testing.assert_array_equal(statsb[:, CMP_B], stbo[:, CMP_B])
    np.testing.assert_array_equal(g, go)
    np.testing.assert_array_equal(lam, lo)
    plain = Solver(prob, abstol=1e-8, reltol=1e-8)
    yp, stp, statsp = plain.solve_batch(0.0, tv, d["y0"], d["ps"], d["pr"])
    orc = make_oracle("bessel_ring")
    ypo, spo, stpo = orc.solve(orc.config(rtol=1e-8, atol=1e-8), d["y0"], d["ps"], d["pr"], 0.0, tv, nthreads=8)
    assert (stp == 0).all() and (spo == 0).all()
    np.testing.assert_array_equal(yp, ypo)
    np.testing.assert_array_equal(statsp[:, CMP[:8]], stpo[:, CMP[:8]])


@pytest.mark.parametrize("group", ["wave4", "wave", "mem"])
def test_bessel_ring_through_the_other_mappings(group, monkeypatch):
    """The callbacks staged through LDS (4-lane groups), run by a 4-wavefront workgroup and out of the HBM workspace:
    still the oracle's bits (B = 70)."""
    from sunode_amd.solver import AdjointSolver
    monkeypatch.setenv("SA_FORCE_GROUP", group)
    prob = make_problem("bessel_ring")
    d, (yo, so, sto), (go, lo, sbo, stbo) = _oracle_run(70)
    tv = d["tvals"]
    sol = AdjointSolver(prob, **TOL)
    y, st, stats = sol.solve_forward_batch(0.0, tv, d["y0"], d["ps"], d["pr"])
    g, lam, stb, statsb = sol.solve_backward_batch(tv[-1], 0.0, tv, d["grads"])
    assert (st == 0).all() and (stb == 0).all()
    np.testing.assert_array_equal(stats[:, CMP], sto[:, CMP])
    np.testing.assert_array_equal(y, yo)
    np.testing.assert_array_equal(statsb[:, CMP_B], stbo[:, CMP_B])
    np.testing.assert_array_equal(g, go)
    np.testing.assert_array_equal(lam, lo)
    sol._engine().close()


def test_bessel_ring_forward_sensitivities():
    """``Solver(sens_mode="simultaneous")`` at B = 64 (5 differentiated parameters x 3 states): states and
    sensitivities equal the oracle's bit for bit."""
    from sunode_amd.solver import Solver
    prob = make_problem("bessel_ring")
    d = bessel_ring_batch(64)
    tv = d["tvals"]
    sol = Solver(prob, abstol=1e-8, reltol=1e-8, sens_mode="simultaneous")
    sens0 = np.zeros((prob.n_params, prob.n_states))
    y, sens, st, stats = sol.solve_sens_batch(0.0, tv, d["y0"], d["ps"], d["pr"], sens0)
    orc = make_oracle("bessel_ring")
    yo, seno, so, sto = orc.solve_sens(orc.config(rtol=1e-8, atol=1e-8), d["y0"], d["ps"], d["pr"], sens0, 0.0, tv,
                                       mode="simultaneous", nthreads=8)
    assert (st == 0).all() and (so == 0).all()
    np.testing.assert_array_equal(y, yo)
    np.testing.assert_array_equal(sens, seno)
    np.testing.assert_array_equal(stats[:, CMP[:8]], sto[:, CMP[:8]])


def test_bessel_ring_matches_truth(golden_dir):
    """Device vs DOP853 truth (tests/golden/truth_bessel_ring.npz, 16 draws): states <= 1e-5, gradients and -lamda
    <= 4e-6 relative to the per-draw maximum."""
    from sunode_amd.solver import AdjointSolver
    d = np.load(os.path.join(golden_dir, "truth_bessel_ring.npz"))
    sol = AdjointSolver(make_problem("bessel_ring"), **TOL)
    tv = d["tvals"]
    y, st, _ = sol.solve_forward_batch(float(d["t0"]), tv, d["y0"], d["ps"], d["pr"])
    g, lam, stb, _ = sol.solve_backward_batch(tv[-1], float(d["t0"]), tv, d["grads"])
    assert (st == 0).all() and (stb == 0).all()
    assert np.max(np.abs(y - d["y_out"]) / np.abs(d["y_out"]).max(axis=(0, 1))) < 1e-5
    assert np.max(np.abs(g - d["grad_params"]) / np.abs(d["grad_params"]).max(axis=1, keepdims=True)) < 4e-6
    assert np.max(np.abs(-lam - d["grad_y0"]) / np.abs(d["grad_y0"]).max(axis=1, keepdims=True)) < 4e-6


def test_an_argument_of_y0_through_zero_is_a_per_instance_failure():
    """g = 6 on one draw of 64 lets z approach 1 + x; -r Y1(1 + x - z) then drives the argument of Y1 and Y0 through
    zero in finite time (-inf there, NaN beyond): that instance reports the oracle's failure status with NaN outputs -- an ordinary solver
    status --, the other 63 equal the oracle bit for bit."""
    from sunode_amd.solver import AdjointSolver
    prob = make_problem("bessel_ring")
    d = bessel_ring_batch(64)
    ps = d["ps"].copy()
    ps[FAIL_DRAW, 2] = FAIL_G
    sol = AdjointSolver(prob, **TOL)
    y, st, _ = sol.solve_forward_batch(0.0, d["tvals"], d["y0"], ps, d["pr"])
    orc = make_oracle("bessel_ring")
    cfg = orc.config(rtol=1e-8, atol=1e-8, rtolB=1e-8, atolB=1e-8, rtolQB=1e-8, atolQB=1e-8)
    yo, so, _ = orc.solve_forward(cfg, d["y0"], ps, d["pr"], 0.0, d["tvals"], nthreads=8)
    assert so[FAIL_DRAW] != 0 and st[FAIL_DRAW] == so[FAIL_DRAW] and np.isnan(y[FAIL_DRAW]).any()
    np.testing.assert_array_equal(st, so)
    ok = st == 0
    assert ok.sum() == 63
    np.testing.assert_array_equal(y[ok], yo[ok])
