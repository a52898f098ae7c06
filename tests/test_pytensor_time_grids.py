"""The pytensor Ops with a start time and an output grid per draw (``SolveODEAdjointBatchTimes`` / ``...Backward`` /
``EvalRhsBatchTimes``): ``perform`` against the solver, and the ``grad`` wiring evaluated through the graph -- d/dtvals
per draw, d/dtvals[b, i] = rhs(t_bi, y_b(t_bi)) . g_bi, and with equal rows the per-draw d/dtvals summed over the batch
equals the shared-grid Op's.  Uses the stub pytensor of tests/stubs when pytensor is absent, as
tests/test_pytensor_ops.py does."""
import importlib
import os
import sys

import numpy as np
import pytest

from tests.helpers import make_problem

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ops():
    try:
        import pytensor  # noqa: F401
        stub = None
    except ImportError:
        stub = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stubs")
        sys.path.insert(0, stub)
    sys.modules.pop("sunode_amd.wrappers.as_pytensor", None)
    mod = importlib.import_module("sunode_amd.wrappers.as_pytensor")
    yield mod
    if stub:
        sys.path.remove(stub)
        for name in [n for n in sys.modules if n == "pytensor" or n.startswith("pytensor.")]:
            del sys.modules[name]
        sys.modules.pop("sunode_amd.wrappers.as_pytensor", None)


def _run(op, inputs, n_out):
    outputs = [[None] for _ in range(n_out)]
    op.perform(None, inputs, outputs)
    return [o[0] for o in outputs]


def _solver():
    from sunode_amd.solver import AdjointSolver
    tol = 1e-9
    return AdjointSolver(make_problem("lv"), abstol=tol, reltol=tol, backward_abstol=tol, backward_reltol=tol,
                         quad_abstol=tol, quad_reltol=tol)


Y0 = np.array([[1.0, 0.1], [1.1, 0.12], [0.9, 0.2]])
P = np.array([[0.1, 0.2], [0.12, 0.18], [0.09, 0.25]])
FIXED = np.array([0.3, 0.4])
T0 = np.array([0.0, 0.25, 0.7])
TV = np.sort(T0[:, None] + np.random.default_rng(2).uniform(0.0, 10.0, (3, 21)), axis=1)
W = np.cos(np.arange(3 * 42.0)).reshape(3, 21, 2)


def test_perform_equals_the_solver(ops):
    solver = _solver()
    y, = _run(ops.SolveODEAdjointBatchTimes(solver), [Y0, P, FIXED, T0, TV], 1)
    lam, grad = _run(ops.SolveODEAdjointBatchTimesBackward(solver), [Y0, P, FIXED, W, T0, TV], 2)
    yd, st, _ = solver.solve_forward_batch(T0, TV, Y0, P, FIXED)
    gd, ld, stb, _ = solver.solve_backward_batch(TV[:, -1], T0, TV, W)
    assert (st == 0).all() and (stb == 0).all()
    np.testing.assert_array_equal(y, yd)
    np.testing.assert_array_equal(grad, gd)
    np.testing.assert_array_equal(lam, ld)
    rhs, = _run(ops.EvalRhsBatchTimes(solver), [P, FIXED, y, TV], 1)
    assert rhs.shape == (3, 21, 2)


def test_grad_per_draw_and_equal_rows_sum_to_the_shared_op(ops):
    pytensor = pytest.importorskip("pytensor")
    if not hasattr(pytensor, "evaluate"):
        pytest.skip("graph evaluation helper of the stub only")
    pt = importlib.import_module("pytensor.tensor")
    solver = _solver()
    y0v, pv = pt.dmatrix("y0"), pt.dmatrix("params")
    givens = {y0v: Y0, pv: P}
    flat = ops.SolveODEAdjointBatchTimes(solver)(y0v, pv, FIXED, T0, TV)
    node = flat.owner
    gl = node.op.grad(node.inputs, [pt.as_tensor_variable(W)])
    assert len(gl) == 5 and type(gl[2]).__name__ == "NotImplementedGrad" and type(gl[3]).__name__ == "NotImplementedGrad"
    y, d_y0, d_params, d_tvals = pytensor.evaluate([flat, gl[0], gl[1], gl[4]], givens)
    assert d_tvals.shape == (3, 21)
    solver.solve_forward_batch(T0, TV, Y0, P, FIXED)
    gd, ld, _, _ = solver.solve_backward_batch(TV[:, -1], T0, TV, W)
    np.testing.assert_array_equal(d_params, gd)
    np.testing.assert_array_equal(d_y0, -ld)
    for b in range(3):                                     # Lotka-Volterra: alpha, beta differentiated; gamma, delta fixed
        rhs = np.stack([P[b, 0] * y[b, :, 0] - P[b, 1] * y[b, :, 1] * y[b, :, 0],
                        FIXED[1] * y[b, :, 0] * y[b, :, 1] - FIXED[0] * y[b, :, 1]], axis=1)
        np.testing.assert_allclose(d_tvals[b], (rhs * W[b]).sum(-1), rtol=1e-12, atol=1e-14)
    # equal rows: the per-draw gradients summed over the batch = the shared-grid Op's d/dtvals
    row = TV[1]
    shared = ops.SolveODEAdjointBatch(solver)(y0v, pv, FIXED, 0.0, row)
    gs = shared.owner.op.grad(shared.owner.inputs, [pt.as_tensor_variable(W)])
    per = ops.SolveODEAdjointBatchTimes(solver)(y0v, pv, FIXED, np.zeros(3), np.tile(row, (3, 1)))
    gp = per.owner.op.grad(per.owner.inputs, [pt.as_tensor_variable(W)])
    ys, dts, yp, dtp = pytensor.evaluate([shared, gs[4], per, gp[4]], givens)
    np.testing.assert_array_equal(yp, ys)
    np.testing.assert_allclose(dtp.sum(0), dts, rtol=1e-14, atol=0)


def _forcing_truth():
    from tests.test_time_grid_truth import load_truth
    return load_truth(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"), "forcing")


def _forcing_solver():
    from sunode_amd.solver import AdjointSolver
    tol = 1e-9
    return AdjointSolver(make_problem("forcing"), abstol=tol, reltol=tol, backward_abstol=tol, backward_reltol=tol,
                         quad_abstol=tol, quad_reltol=tol)


def _rel_rows(got, want):
    return np.max(np.abs(got - want) / np.abs(want).max(axis=1, keepdims=True))


def test_eval_rhs_reads_each_draws_own_times(ops):
    """EvalRhsBatchTimes.perform on ``forcing`` (its right-hand side reads t) at the truth's states and per-draw grids:
    rhs . g equals the fixture's d_tvals (tests/golden/truth_times_forcing.npz) -- a time column in the wrong order or
    tiled from one row would not."""
    t = _forcing_truth()
    rhs, = _run(ops.EvalRhsBatchTimes(_forcing_solver()), [t["ps"], t["pr"], t["y_out"], t["tvals"]], 1)
    assert rhs.shape == t["y_out"].shape
    assert _rel_rows((rhs * t["grads"]).sum(-1), t["d_tvals"]) < 1e-5


def test_graph_d_tvals_of_a_time_dependent_model_vs_truth(ops):
    """The graph's d/dtvals of SolveODEAdjointBatchTimes on ``forcing`` with the fixture's per-draw t0 / tvals against
    the truth's d_tvals = f(t_bk, y_b(t_bk)) . g_bk."""
    pytensor = pytest.importorskip("pytensor")
    if not hasattr(pytensor, "evaluate"):
        pytest.skip("graph evaluation helper of the stub only")
    pt = importlib.import_module("pytensor.tensor")
    t = _forcing_truth()
    y0v, pv = pt.dmatrix("y0"), pt.dmatrix("params")
    flat = ops.SolveODEAdjointBatchTimes(_forcing_solver())(y0v, pv, t["pr"], t["t0"], t["tvals"])
    gl = flat.owner.op.grad(flat.owner.inputs, [pt.as_tensor_variable(t["grads"])])
    d_tvals, = pytensor.evaluate([gl[4]], {y0v: t["y0"], pv: t["ps"]})
    assert d_tvals.shape == t["d_tvals"].shape
    assert _rel_rows(d_tvals, t["d_tvals"]) < 1e-5
