"""The checks every function family makes on its models, written once (a plain module: no fixtures, no tests).

The GPU tests of a family (tests/test_gpu_inverse_erf.py, test_gpu_gamma.py, test_gpu_bessel.py, test_gpu_transcendental.py)
keep their points, argument tables, bars and docstrings and call these bodies with the name of a model of
tools/family_models.py; the CPU math tests compile their block headers through ``compile_math_blocks``.  All solves run
at rtol = atol = 1e-8 (``TOL``).
"""
import ctypes
import functools
import hashlib
import os
import subprocess

import numpy as np

from tests.helpers import make_oracle, make_problem
from tools.family_models import FAMILY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CMP = [0, 1, 2, 3, 4, 5, 6, 7, 8]                      # forward statistics compared with the oracle's
CMP_B = [0, 1, 2, 3, 4, 5, 6, 9, 10, 12]               # ... and backward
TOL = dict(abstol=1e-8, reltol=1e-8, backward_abstol=1e-8, backward_reltol=1e-8, quad_abstol=1e-8, quad_reltol=1e-8)
KEYS = ("rhs", "jac", "adj", "quad", "adjjac")


def _adjoint_config(orc):
    return orc.config(rtol=1e-8, atol=1e-8, rtolB=1e-8, atolB=1e-8, rtolQB=1e-8, atolQB=1e-8)


@functools.lru_cache(maxsize=None)
def oracle_run(model, B):
    """Forward + adjoint of the B-draw batch of ``model`` in the oracle (computed once per model and batch size)."""
    d = FAMILY[model].batch(B)
    orc = make_oracle(model)
    cfg = _adjoint_config(orc)
    tv = d["tvals"]
    fwd = orc.solve_forward(cfg, d["y0"], d["ps"], d["pr"], 0.0, tv, nthreads=8)
    bwd = orc.solve_backward(cfg, tv[-1], 0.0, tv, d["grads"], nthreads=8)
    return d, fwd, bwd


def callbacks_equal_host_bitwise(model, y, par, lam, t):
    """The generated callbacks of ``model`` at the points (t, y, lam, par): all five callbacks and the return codes are the
    host's, bit for bit.  Two NaNs count as equal, so at least 60 % of the points of every output must be finite in the
    oracle -- NaN == NaN cannot carry the comparison -- and at least one must not be."""
    from sunode_amd.solver import Solver
    eng = Solver(make_problem(model))._engine()
    orc = make_oracle(model)
    N = len(t)
    with np.errstate(all="ignore"):
        got = eng.eval_callbacks(t, y, lam, par, np.zeros((N, 0)))
    differing = 0
    finite = {key: 0 for key in KEYS}
    for i in range(N):
        host = orc.eval(t[i], y[i], lam[i], par[i], np.zeros(0))
        for key in KEYS:
            a, b = np.asarray(got[key][i]).ravel(), np.asarray(host[key]).ravel()
            differing += int(np.sum((a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))))
            finite[key] = finite[key] + np.isfinite(b)
        assert got["codes"][i].tolist() == np.asarray(host["codes"]).tolist()
    assert differing == 0
    for key in KEYS:
        assert (finite[key] >= 0.6 * N).all(), (key, finite[key] / N)
        assert (finite[key] < N).any(), key


def _adjoint_equals_oracle(sol, d, fwd, bwd):
    """Forward + backward solve of ``sol`` on the batch ``d``: no failure, statistics and outputs are the oracle's."""
    (yo, so, sto), (go, lo, sbo, stbo) = fwd, bwd
    tv = d["tvals"]
    y, st, stats = sol.solve_forward_batch(0.0, tv, d["y0"], d["ps"], d["pr"])
    g, lam, stb, statsb = sol.solve_backward_batch(tv[-1], 0.0, tv, d["grads"])
    assert (st == 0).all() and (stb == 0).all()
    np.testing.assert_array_equal(stats[:, CMP], sto[:, CMP])
    np.testing.assert_array_equal(y, yo)
    np.testing.assert_array_equal(statsb[:, CMP_B], stbo[:, CMP_B])
    np.testing.assert_array_equal(g, go)
    np.testing.assert_array_equal(lam, lo)


def forward_adjoint_bitexact(model, B):
    """Statuses, step / order counters and every output equal the oracle's bit for bit, through AdjointSolver and the
    plain Solver."""
    from sunode_amd.solver import AdjointSolver, Solver
    prob = make_problem(model)
    d, fwd, bwd = oracle_run(model, B)
    assert (fwd[1] == 0).all() and (bwd[2] == 0).all()
    _adjoint_equals_oracle(AdjointSolver(prob, **TOL), d, fwd, bwd)
    tv = d["tvals"]
    yp, stp, statsp = Solver(prob, abstol=1e-8, reltol=1e-8).solve_batch(0.0, tv, d["y0"], d["ps"], d["pr"])
    orc = make_oracle(model)
    ypo, spo, stpo = orc.solve(orc.config(rtol=1e-8, atol=1e-8), d["y0"], d["ps"], d["pr"], 0.0, tv, nthreads=8)
    assert (stp == 0).all() and (spo == 0).all()
    np.testing.assert_array_equal(yp, ypo)
    np.testing.assert_array_equal(statsp[:, CMP[:8]], stpo[:, CMP[:8]])


def through_mapping(model, B, group, monkeypatch):
    """Forward + adjoint with the mapping ``group`` forced: still the oracle's bits."""
    from sunode_amd.solver import AdjointSolver
    monkeypatch.setenv("SA_FORCE_GROUP", group)
    sol = AdjointSolver(make_problem(model), **TOL)
    _adjoint_equals_oracle(sol, *oracle_run(model, B))
    sol._engine().close()


def forward_sens_bitexact(model, B, mode):
    """``Solver(sens_mode=mode)``: states, sensitivities and statistics equal the oracle's bit for bit.  Returns the
    sensitivities."""
    from sunode_amd.solver import Solver
    prob = make_problem(model)
    d = FAMILY[model].batch(B)
    tv = d["tvals"]
    sol = Solver(prob, abstol=1e-8, reltol=1e-8, sens_mode=mode)
    sens0 = np.zeros((prob.n_params, prob.n_states))
    y, sens, st, stats = sol.solve_sens_batch(0.0, tv, d["y0"], d["ps"], d["pr"], sens0)
    orc = make_oracle(model)
    yo, seno, so, sto = orc.solve_sens(orc.config(rtol=1e-8, atol=1e-8), d["y0"], d["ps"], d["pr"], sens0, 0.0, tv,
                                       mode=mode, nthreads=8)
    assert (st == 0).all() and (so == 0).all()
    np.testing.assert_array_equal(y, yo)
    np.testing.assert_array_equal(sens, seno)
    np.testing.assert_array_equal(stats[:, CMP[:8]], sto[:, CMP[:8]])
    return sens


def matches_truth(model, golden_dir, bars):
    """Device vs DOP853 truth (tests/golden/truth_<model>.npz): states below ``bars["y"]`` relative to the component's
    maximum, gradients and -lamda below ``bars["grad"]`` relative to the per-draw maximum."""
    from sunode_amd.solver import AdjointSolver
    d = np.load(os.path.join(golden_dir, "truth_%s.npz" % model))
    assert len(d["y0"]) == FAMILY[model].truth_draws
    sol = AdjointSolver(make_problem(model), **TOL)
    tv = d["tvals"]
    y, st, _ = sol.solve_forward_batch(float(d["t0"]), tv, d["y0"], d["ps"], d["pr"])
    g, lam, stb, _ = sol.solve_backward_batch(tv[-1], float(d["t0"]), tv, d["grads"])
    assert (st == 0).all() and (stb == 0).all()
    assert np.max(np.abs(y - d["y_out"]) / np.abs(d["y_out"]).max(axis=(0, 1))) < bars["y"]
    assert np.max(np.abs(g - d["grad_params"]) / np.abs(d["grad_params"]).max(axis=1, keepdims=True)) < bars["grad"]
    assert np.max(np.abs(-lam - d["grad_y0"]) / np.abs(d["grad_y0"]).max(axis=1, keepdims=True)) < bars["grad"]


def per_instance_failure(model, draw, column, value):
    """Differentiated parameter ``column`` of one draw of 64 set to ``value``: that instance reports the oracle's failure
    status with NaN outputs -- an ordinary solver status --, the other 63 equal the oracle bit for bit."""
    from sunode_amd.solver import AdjointSolver
    d = FAMILY[model].batch(64)
    ps = d["ps"].copy()
    ps[draw, column] = value
    y, st, _ = AdjointSolver(make_problem(model), **TOL).solve_forward_batch(0.0, d["tvals"], d["y0"], ps, d["pr"])
    orc = make_oracle(model)
    yo, so, _ = orc.solve_forward(_adjoint_config(orc), d["y0"], ps, d["pr"], 0.0, d["tvals"], nthreads=8)
    assert so[draw] != 0 and st[draw] == so[draw] and np.isnan(y[draw]).any()
    np.testing.assert_array_equal(st, so)
    ok = st == 0
    assert ok.sum() == 63
    np.testing.assert_array_equal(y[ok], yo[ok])


def compile_math_blocks(blocks, wrappers):
    """The headers of the blocks ``blocks`` of codegen.MATH_BLOCKS and the C functions ``wrappers`` (what a test calls
    through ctypes), compiled for the host exactly like the oracle compiles a generated header -> ctypes.CDLL."""
    from sunode_amd.symode.codegen import MATH_BLOCKS
    hdrs = [os.path.join(ROOT, "sunode_amd", "csrc", block.header) for block in MATH_BLOCKS if block.name in blocks]
    assert len(hdrs) == len(blocks)
    key = hashlib.sha256(b"".join(open(h, "rb").read() for h in hdrs) + "\n".join(wrappers).encode()).hexdigest()[:12]
    out = os.path.join(ROOT, "oracle", "_build", "sa_math_%s_%s.so" % (blocks[-1], key))
    if not os.path.exists(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        src = ["#include <math.h>", "#define SA_FN static inline"] + ['#include "%s"' % h for h in hdrs] + list(wrappers)
        c = out[:-3] + ".c"
        with open(c, "w") as fh:
            fh.write("\n".join(src) + "\n")
        with open("/proc/cpuinfo") as fh:
            fma = ["-mfma"] if " fma " in fh.read() else []
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-std=gnu11"] + fma +
                       [c, "-o", out, "-lm"], check=True, capture_output=True, text=True)
    return ctypes.CDLL(out)
