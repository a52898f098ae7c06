"""Inverse trigonometric / inverse hyperbolic functions and erf / erfc on the device (pytest -m gpu).

Models (tools/problems.py): ``mathfn_c`` (asin / acos / atan / atan2) and ``mathfn_d`` (asinh / acosh / atanh / erf /
erfc) -- one or two functions of csrc/sa_math_inv.h per output, a state times or over a differentiated parameter as
the argument; ``probit_gate`` -- all nine in one integrated right-hand side (callbacks pinned by hand-written closed
forms and the truth fixture, tests/test_inverse_erf_math.py).

Bars: device == oracle BIT FOR BIT (statuses, counters, every fp64 output) -- the generated header embeds
csrc/sa_math.h and csrc/sa_math_inv.h, so host and device execute one IEEE operation sequence; device vs DOP853 truth
at the bars of tests/test_gpu_transcendental.py (states <= 1e-5, gradients <= 4e-6 relative at rtol = atol = 1e-8).
"""
import functools
import os

import numpy as np
import pytest

from tests.helpers import make_oracle, make_problem
from tools.problems import probit_gate_batch

pytestmark = pytest.mark.gpu

CMP = [0, 1, 2, 3, 4, 5, 6, 7, 8]
CMP_B = [0, 1, 2, 3, 4, 5, 6, 9, 10, 12]
TOL = dict(abstol=1e-8, reltol=1e-8, backward_abstol=1e-8, backward_reltol=1e-8, quad_abstol=1e-8, quad_reltol=1e-8)


@functools.lru_cache(maxsize=None)
def _oracle_run(B):
    """Forward + adjoint of the B-draw batch of ``probit_gate`` in the oracle (computed once per batch size)."""
    d = probit_gate_batch(B)
    orc = make_oracle("probit_gate")
    cfg = orc.config(rtol=1e-8, atol=1e-8, rtolB=1e-8, atolB=1e-8, rtolQB=1e-8, atolQB=1e-8)
    tv = d["tvals"]
    fwd = orc.solve_forward(cfg, d["y0"], d["ps"], d["pr"], 0.0, tv, nthreads=8)
    bwd = orc.solve_backward(cfg, tv[-1], 0.0, tv, d["grads"], nthreads=8)
    return d, fwd, bwd


def _points(name, N):
    """States and parameters that put the arguments into EVERY interval of every function (the boundaries:
    codegen.math_inv_boundaries()) and, for a minority of the points, outside the domains."""
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
    from sunode_amd.solver import Solver
    prob = make_problem(name)
    eng = Solver(prob)._engine()
    orc = make_oracle(name)
    N = 4096
    y, par, lam, t = _points(name, N)
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
        assert (finite[key] < N).any(), key           # (and some arguments were outside a domain)


def test_probit_gate_forward_adjoint_bitexact_vs_oracle():
    """B = 300 (four full wavefronts and a ragged one): statuses, step / order counters and every output equal the
    oracle's bit for bit, through AdjointSolver and the plain Solver."""
    from sunode_amd.solver import AdjointSolver, Solver
    prob = make_problem("probit_gate")
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
    orc = make_oracle("probit_gate")
    ypo, spo, stpo = orc.solve(orc.config(rtol=1e-8, atol=1e-8), d["y0"], d["ps"], d["pr"], 0.0, tv, nthreads=8)
    assert (stp == 0).all() and (spo == 0).all()
    np.testing.assert_array_equal(yp, ypo)
    np.testing.assert_array_equal(statsp[:, CMP[:8]], stpo[:, CMP[:8]])


@pytest.mark.parametrize("group", ["wave4", "wave", "mem"])
def test_probit_gate_through_the_other_mappings(group, monkeypatch):
    """The callbacks staged through LDS (4-lane groups), run by a 4-wavefront workgroup and out of the HBM workspace:
    still the oracle's bits (B = 70)."""
    from sunode_amd.solver import AdjointSolver
    monkeypatch.setenv("SA_FORCE_GROUP", group)
    prob = make_problem("probit_gate")
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


def test_probit_gate_forward_sensitivities():
    """``Solver(sens_mode="simultaneous")`` at B = 64 (5 differentiated parameters x 3 states): states and
    sensitivities equal the oracle's bit for bit."""
    from sunode_amd.solver import Solver
    prob = make_problem("probit_gate")
    d = probit_gate_batch(64)
    tv = d["tvals"]
    sol = Solver(prob, abstol=1e-8, reltol=1e-8, sens_mode="simultaneous")
    sens0 = np.zeros((prob.n_params, prob.n_states))
    y, sens, st, stats = sol.solve_sens_batch(0.0, tv, d["y0"], d["ps"], d["pr"], sens0)
    orc = make_oracle("probit_gate")
    yo, seno, so, sto = orc.solve_sens(orc.config(rtol=1e-8, atol=1e-8), d["y0"], d["ps"], d["pr"], sens0, 0.0, tv,
                                       mode="simultaneous", nthreads=8)
    assert (st == 0).all() and (so == 0).all()
    np.testing.assert_array_equal(y, yo)
    np.testing.assert_array_equal(sens, seno)
    np.testing.assert_array_equal(stats[:, CMP[:8]], sto[:, CMP[:8]])


def test_probit_gate_matches_truth(golden_dir):
    """Device vs DOP853 truth (tests/golden/truth_probit_gate.npz, 16 draws): states <= 1e-5, gradients and -lamda
    <= 4e-6 relative to the per-draw maximum."""
    from sunode_amd.solver import AdjointSolver
    d = np.load(os.path.join(golden_dir, "truth_probit_gate.npz"))
    sol = AdjointSolver(make_problem("probit_gate"), **TOL)
    tv = d["tvals"]
    y, st, _ = sol.solve_forward_batch(float(d["t0"]), tv, d["y0"], d["ps"], d["pr"])
    g, lam, stb, _ = sol.solve_backward_batch(tv[-1], float(d["t0"]), tv, d["grads"])
    assert (st == 0).all() and (stb == 0).all()
    assert np.max(np.abs(y - d["y_out"]) / np.abs(d["y_out"]).max(axis=(0, 1))) < 1e-5
    assert np.max(np.abs(g - d["grad_params"]) / np.abs(d["grad_params"]).max(axis=1, keepdims=True)) < 4e-6
    assert np.max(np.abs(-lam - d["grad_y0"]) / np.abs(d["grad_y0"]).max(axis=1, keepdims=True)) < 4e-6


def test_out_of_domain_argument_is_a_per_instance_failure():
    """b = 4 on one draw of 64 drives asin(b x / (1 + z)) beyond 1: that instance reports the oracle's failure status
    with NaN outputs -- an ordinary solver status --, the other 63 equal the oracle bit for bit."""
    from sunode_amd.solver import AdjointSolver
    prob = make_problem("probit_gate")
    d = probit_gate_batch(64)
    ps = d["ps"].copy()
    ps[5, 4] = 4.0
    sol = AdjointSolver(prob, **TOL)
    y, st, _ = sol.solve_forward_batch(0.0, d["tvals"], d["y0"], ps, d["pr"])
    orc = make_oracle("probit_gate")
    cfg = orc.config(rtol=1e-8, atol=1e-8, rtolB=1e-8, atolB=1e-8, rtolQB=1e-8, atolQB=1e-8)
    yo, so, _ = orc.solve_forward(cfg, d["y0"], ps, d["pr"], 0.0, d["tvals"], nthreads=8)
    assert so[5] != 0 and st[5] == so[5] and np.isnan(y[5]).any()
    np.testing.assert_array_equal(st, so)
    ok = st == 0
    assert ok.sum() == 63
    np.testing.assert_array_equal(y[ok], yo[ok])
