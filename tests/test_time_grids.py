"""Per-instance start times and output grids (include/sunode_amd.h sa_*_batch_times): the C ABI and the shape checks
of the batch methods, which run before any device work (tests/test_gpu_time_grids.py covers the results)."""
import os
import re

import numpy as np
import pytest

from tests.helpers import make_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sa_solve_batch_times", "sa_solve_sens_batch_times", "sa_solve_forward_batch_times",
         "sa_solve_backward_batch_times")


def test_entry_points_are_declared_and_exported():
    from sunode_amd import _native
    header = open(os.path.join(ROOT, "include", "sunode_amd.h")).read()
    declared = set(re.findall(r"\b(sa_[a-z_]+)\s*\(", header))
    L = _native.load_library()
    for name in NAMES:
        assert name in declared and name in _native.EXPORTED_SYMBOLS and hasattr(L, name), name


def test_per_instance_kernels_in_every_code_object_family():
    """Both launch forms of each kernel body: the shared-time kernels the budget holds, and the *_t kernels."""
    for f in ("bdf_kernels.hip", "bdf_wave.hip", "bdf_mem.hip"):
        src = open(os.path.join(ROOT, "sunode_amd", "csrc", f)).read()
        for k in ("sa_k_forward", "sa_k_backward", "sa_k_sens"):
            assert re.search(r"\b%s\(" % k, src) and re.search(r"\b%s_t\(" % k, src), (f, k)


def _lv():
    prob = make_problem("lv")
    B = 5
    y0 = np.ones((B, 2))
    ps = np.ones((B, prob.n_params))
    pr = np.ones(prob.n_remainder)
    return prob, B, y0, ps, pr


def _no_engine(sol, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("device work before the shape check")
    monkeypatch.setattr(type(sol), "_engines", refuse)
    return sol


BAD = [
    ("t0 length", lambda B: (np.zeros(B + 1), np.tile(np.linspace(1, 2, 4), (B, 1)))),
    ("grid rows", lambda B: (0.0, np.tile(np.linspace(1, 2, 4), (B + 2, 1)))),
    ("3-d grid", lambda B: (0.0, np.zeros((B, 4, 1)))),
    ("2-d t0", lambda B: (np.zeros((B, 1)), np.linspace(1, 2, 4))),
    ("empty rows", lambda B: (np.zeros(B), np.zeros((B, 0)))),
]


@pytest.mark.parametrize("case", [c[0] for c in BAD])
def test_shape_errors_raise_before_device_work(case, monkeypatch):
    from sunode_amd.solver import AdjointSolver, Solver
    make = dict(BAD)[case]
    prob, B, y0, ps, pr = _lv()
    t0, tv = make(B)
    with pytest.raises(ValueError):
        _no_engine(Solver(prob), monkeypatch).solve_batch(t0, tv, y0, ps, pr)
    with pytest.raises(ValueError):
        _no_engine(Solver(prob, sens_mode="simultaneous"), monkeypatch).solve_sens_batch(
            t0, tv, y0, ps, pr, np.zeros((prob.n_params, 2)))
    with pytest.raises(ValueError):
        _no_engine(AdjointSolver(prob), monkeypatch).solve_forward_batch(t0, tv, y0, ps, pr)


def test_backward_shape_errors(monkeypatch):
    from sunode_amd.solver import AdjointSolver
    prob, B, y0, ps, pr = _lv()
    sol = _no_engine(AdjointSolver(prob), monkeypatch)
    sol._last_forward = (B, ps, pr, 0, [], None)          # as after a forward call of B instances
    tv = np.tile(np.linspace(1, 2, 4), (B, 1))
    for t0, tend, grid in ((np.ones(B), np.zeros(B + 1), tv), (np.ones(B - 1), 0.0, tv), (2.0, 0.0, tv[:2]),
                           (2.0, np.zeros((B, 2)), tv)):
        with pytest.raises(ValueError):
            sol.solve_backward_batch(t0, tend, grid, np.ones((4, 2)))


def test_shared_times_take_the_plain_path():
    from sunode_amd.solver import Solver
    prob, B, *_ = _lv()
    got = Solver(prob)._time_args(B, 0.5, [1.0, 2.0])
    assert got[1] is None and got[6] is None and got[7] is False and got[0] == 0.5
    got = Solver(prob)._time_args(B, 0.5, np.ones((B, 3)))
    assert got[1] is None and got[6] == 3 and got[7] is True


def test_a_scalar_grid_is_one_output_time():
    from sunode_amd.solver import Solver
    prob, B, *_ = _lv()
    got = Solver(prob)._time_args(B, 0.0, 5.0)
    assert got[4].shape == (1,) and got[5] == 1 and got[7] is False
