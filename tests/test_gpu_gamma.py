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
import functools
import os

import numpy as np
import pytest

from tests.helpers import make_oracle, make_problem
from tools.problems import gamma_delay_batch

pytestmark = pytest.mark.gpu

CMP = [0, 1, 2, 3, 4, 5, 6, 7, 8]
CMP_B = [0, 1, 2, 3, 4, 5, 6, 9, 10, 12]
TOL = dict(abstol=1e-8, reltol=1e-8, backward_abstol=1e-8, backward_reltol=1e-8, quad_abstol=1e-8, quad_reltol=1e-8)


@functools.lru_cache(maxsize=None)
def _oracle_run(B):
    """Forward + adjoint of the B-draw batch of ``gamma_delay`` in the oracle (computed once per batch size)."""
    d = gamma_delay_batch(B)
    orc = make_oracle("gamma_delay")
    cfg = orc.config(rtol=1e-8, atol=1e-8, rtolB=1e-8, atolB=1e-8, rtolQB=1e-8, atolQB=1e-8)
    tv = d["tvals"]
    fwd = orc.solve_forward(cfg, d["y0"], d["ps"], d["pr"], 0.0, tv, nthreads=8)
    bwd = orc.solve_backward(cfg, tv[-1], 0.0, tv, d["grads"], nthreads=8)
    return d, fwd, bwd


def _points(N):
    """States and parameters of ``mathfn_e`` that put the arguments into EVERY piece of every function (the boundaries:
    codegen.math_gamma_boundaries()), onto the negative axis (a negative parameter) and, for one point in 32, exactly
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
    bounds = codegen.math_gamma_boundaries()
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
    from sunode_amd.solver import Solver
    prob = make_problem("mathfn_e")
    eng = Solver(prob)._engine()
    orc = make_oracle("mathfn_e")
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
        assert (finite[key] < N).any(), key           # (and some arguments were on a pole or beyond the overflow)


def test_gamma_delay_forward_adjoint_bitexact_vs_oracle():
    """B = 300 (four full wavefronts and a ragged one): statuses, step / order counters and every output equal the
    oracle's bit for bit, through AdjointSolver and the plain Solver."""
    from sunode_amd.solver import AdjointSolver, Solver
    prob = make_problem("gamma_delay")
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
    orc = make_oracle("gamma_delay")
    ypo, spo, stpo = orc.solve(orc.config(rtol=1e-8, atol=1e-8), d["y0"], d["ps"], d["pr"], 0.0, tv, nthreads=8)
    assert (stp == 0).all() and (spo == 0).all()
    np.testing.assert_array_equal(yp, ypo)
    np.testing.assert_array_equal(statsp[:, CMP[:8]], stpo[:, CMP[:8]])


@pytest.mark.parametrize("group", ["wave4", "wave", "mem"])
def test_gamma_delay_through_the_other_mappings(group, monkeypatch):
    """The callbacks staged through LDS (4-lane groups), run by a 4-wavefront workgroup and out of the HBM workspace:
    still the oracle's bits (B = 70)."""
    from sunode_amd.solver import AdjointSolver
    monkeypatch.setenv("SA_FORCE_GROUP", group)
    prob = make_problem("gamma_delay")
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


def test_gamma_delay_forward_sensitivities():
    """``Solver(sens_mode="simultaneous")`` at B = 64 (5 differentiated parameters x 3 states): states and
    sensitivities equal the oracle's bit for bit."""
    from sunode_amd.solver import Solver
    prob = make_problem("gamma_delay")
    d = gamma_delay_batch(64)
    tv = d["tvals"]
    sol = Solver(prob, abstol=1e-8, reltol=1e-8, sens_mode="simultaneous")
    sens0 = np.zeros((prob.n_params, prob.n_states))
    y, sens, st, stats = sol.solve_sens_batch(0.0, tv, d["y0"], d["ps"], d["pr"], sens0)
    orc = make_oracle("gamma_delay")
    yo, seno, so, sto = orc.solve_sens(orc.config(rtol=1e-8, atol=1e-8), d["y0"], d["ps"], d["pr"], sens0, 0.0, tv,
                                       mode="simultaneous", nthreads=8)
    assert (st == 0).all() and (so == 0).all()
    np.testing.assert_array_equal(y, yo)
    np.testing.assert_array_equal(sens, seno)
    np.testing.assert_array_equal(stats[:, CMP[:8]], sto[:, CMP[:8]])


def test_gamma_delay_matches_truth(golden_dir):
    """Device vs DOP853 truth (tests/golden/truth_gamma_delay.npz, 16 draws): states <= 1e-5, gradients and -lamda
    <= 4e-6 relative to the per-draw maximum."""
    from sunode_amd.solver import AdjointSolver
    d = np.load(os.path.join(golden_dir, "truth_gamma_delay.npz"))
    sol = AdjointSolver(make_problem("gamma_delay"), **TOL)
    tv = d["tvals"]
    y, st, _ = sol.solve_forward_batch(float(d["t0"]), tv, d["y0"], d["ps"], d["pr"])
    g, lam, stb, _ = sol.solve_backward_batch(tv[-1], float(d["t0"]), tv, d["grads"])
    assert (st == 0).all() and (stb == 0).all()
    assert np.max(np.abs(y - d["y_out"]) / np.abs(d["y_out"]).max(axis=(0, 1))) < 1e-5
    assert np.max(np.abs(g - d["grad_params"]) / np.abs(d["grad_params"]).max(axis=1, keepdims=True)) < 4e-6
    assert np.max(np.abs(-lam - d["grad_y0"]) / np.abs(d["grad_y0"]).max(axis=1, keepdims=True)) < 4e-6


def test_reaching_the_pole_is_a_per_instance_failure():
    """b = 6 on one draw of 64 drives 1 - b x into the pole of Gamma at 0 (a finite-time blow-up of x): that instance
    reports the oracle's failure status with NaN outputs -- an ordinary solver status --, the other 63 equal the oracle
    bit for bit."""
    from sunode_amd.solver import AdjointSolver
    prob = make_problem("gamma_delay")
    d = gamma_delay_batch(64)
    ps = d["ps"].copy()
    ps[5, 2] = 6.0
    sol = AdjointSolver(prob, **TOL)
    y, st, _ = sol.solve_forward_batch(0.0, d["tvals"], d["y0"], ps, d["pr"])
    orc = make_oracle("gamma_delay")
    cfg = orc.config(rtol=1e-8, atol=1e-8, rtolB=1e-8, atolB=1e-8, rtolQB=1e-8, atolQB=1e-8)
    yo, so, _ = orc.solve_forward(cfg, d["y0"], ps, d["pr"], 0.0, d["tvals"], nthreads=8)
    assert so[5] != 0 and st[5] == so[5] and np.isnan(y[5]).any()
    np.testing.assert_array_equal(st, so)
    ok = st == 0
    assert ok.sum() == 63
    np.testing.assert_array_equal(y[ok], yo[ok])
