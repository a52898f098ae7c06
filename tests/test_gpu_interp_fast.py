"""-DSA_INTERP_FAST=1 (csrc/bdf_kernels.hip): the one-index move of the backward interpolation as straight-line code,
the look-ahead touches issued after the evaluation, the forward kernel's output time in a register.

None of it may change a bit: Lotka-Volterra through NativeSolver with the -DSA_INTERP_FAST=1 build against the
-DSA_INTERP_FAST=0 build -- states, gradients, adjoint states, both status arrays and all 16 statistics columns of both
passes (the interpolation / rebuild counters and the wavefront's iteration count included) -- and against the CPU
oracle, which walks like CVAfindIndex (outputs, statuses, and the counters the oracle keeps: CMP / CMP_B of
tests/test_gpu_parity.py; it has no attempt count and no wavefront).

Tolerances chosen for the paths of the index search: a coarse forward pass under a tight backward pass (many backward
steps per stored point: moves by zero and one), a tight forward pass under a coarse backward pass (backward steps jump
over several stored points, rejected attempts step back to the right: the walk), the benchmark's 1e-8 everywhere; one
full and one partial wavefront; the per-instance-times launch form (sa_k_backward_t).  The classification itself:
tests/test_interp_fast_move.py."""
import functools

import numpy as np
import pytest

from tests.helpers import make_oracle, make_problem
from tools.problems import lv_batch

pytestmark = pytest.mark.gpu

CMP = [0, 1, 2, 3, 4, 5, 6, 7, 8]            # as tests/test_gpu_parity.py
CMP_B = [0, 1, 2, 3, 4, 5, 6, 9, 10, 12]
N_T = 5
TOLS = {"coarse-forward": (1e-3, 1e-10), "coarse-backward": (1e-10, 1e-4), "bench": (1e-8, 1e-8)}


def _data(B, per_instance):
    prob = make_problem("lv")
    d = lv_batch(B)
    ps = np.ascontiguousarray(d["params"][:, prob.params_subset.subset_index])
    pr = np.ascontiguousarray(d["params"][:, prob.params_subset.remainder_index])
    y0 = np.ascontiguousarray(d["y0"])
    grads = 1.0 + 0.5 * np.cos(1.7 * np.arange(N_T)[:, None] + 0.9 * np.arange(2)[None, :])
    if per_instance:
        rng = np.random.default_rng(11)
        t0 = rng.uniform(0.0, 1.0, B)
        tv = np.sort(t0[:, None] + rng.uniform(0.0, 10.0, (B, N_T)), axis=1)
        tv[::7, 0] = t0[::7]                               # some rows start exactly at t0
    else:
        t0, tv = 0.0, np.linspace(0.0, 10.0, N_T)
    return prob, y0, ps, pr, t0, np.ascontiguousarray(tv), grads


def _device(tols, B, per_instance, defines, monkeypatch):
    """y, status, stats, grad, lamda, status_b, stats_b of one build"""
    from sunode_amd import _native
    prob, y0, ps, pr, t0, tv, grads = _data(B, per_instance)
    tf, tb = TOLS[tols]
    monkeypatch.setenv("SA_KERNEL_DEFINES", defines)
    eng = _native.NativeSolver(prob.native_source(), device=0, n_states=2, guard=False, rtol=tf, atol=tf, rtolB=tb,
                               atolB=tb, rtolQB=tb, atolQB=tb, traj_capacity=4096)
    y = np.zeros((B, N_T, 2)); st = np.zeros(B, np.int32); sc = np.zeros((B, 16), np.int64)
    g = np.zeros((B, 2)); lam = np.zeros((B, 2)); stb = np.zeros(B, np.int32); scb = np.zeros((B, 16), np.int64)
    H = _native.SA_MEM_HOST
    if per_instance:
        t0 = np.ascontiguousarray(t0); tend = np.ascontiguousarray(tv[:, -1])
        eng.solve(H, B, y0, ps, pr, pr.shape[1], t0, tv, N_T, y, st, sc, adjoint=True, t0_stride=1, tvals_stride=N_T)
        eng.solve_backward(H, B, ps, pr, pr.shape[1], tend, t0, tv, N_T, grads, 0, g, lam, stb, scb,
                           t0_stride=1, tend_stride=1, tvals_stride=N_T)
    else:
        eng.solve(H, B, y0, ps, pr, pr.shape[1], t0, tv, N_T, y, st, sc, adjoint=True)
        eng.solve_backward(H, B, ps, pr, pr.shape[1], float(tv[-1]), t0, tv, N_T, grads, 0, g, lam, stb, scb)
    eng.close()
    return y, st, sc, g, lam, stb, scb


@functools.lru_cache(maxsize=None)
def _oracle(tols, B, per_instance):
    prob, y0, ps, pr, t0, tv, grads = _data(B, per_instance)
    tf, tb = TOLS[tols]
    orc = make_oracle("lv")
    cfg = orc.config(rtol=tf, atol=tf, rtolB=tb, atolB=tb, rtolQB=tb, atolQB=tb)
    if not per_instance:
        y, st, sc = orc.solve_forward(cfg, y0, ps, pr, t0, tv)
        g, lam, stb, scb = orc.solve_backward(cfg, tv[-1], t0, tv, grads)
        return y, st, sc, g, lam, stb, scb
    rows = []
    for b in range(B):
        y, st, sc = orc.solve_forward(cfg, y0[b:b + 1], ps[b:b + 1], pr[b:b + 1], float(t0[b]), tv[b])
        g, lam, stb, scb = orc.solve_backward(cfg, tv[b][-1], float(t0[b]), tv[b], grads)
        rows.append((y, st, sc, g, lam, stb, scb))
    return tuple(np.concatenate(c) for c in zip(*rows))


NAMES = ["y_out", "status", "stats", "grad_out", "lamda_out", "status_b", "stats_b"]


def _check(tols, B, per_instance, monkeypatch):
    fast = _device(tols, B, per_instance, "-DSA_INTERP_FAST=1", monkeypatch)
    plain = _device(tols, B, per_instance, "-DSA_INTERP_FAST=0", monkeypatch)
    assert (fast[1] == 0).all() and (fast[5] == 0).all()
    for name, a, b in zip(NAMES, fast, plain):              # every statistics column
        np.testing.assert_array_equal(a, b, err_msg="%s: -DSA_INTERP_FAST=1 against -DSA_INTERP_FAST=0" % name)
    for k, (name, a, b) in enumerate(zip(NAMES, fast, _oracle(tols, B, per_instance))):
        if k in (2, 6):
            a, b = a[:, CMP if k == 2 else CMP_B], b[:, CMP if k == 2 else CMP_B]
        np.testing.assert_array_equal(a, b, err_msg="%s: -DSA_INTERP_FAST=1 against the oracle" % name)
    return fast


@pytest.mark.parametrize("B", [1, 65, 256])
@pytest.mark.parametrize("tols", list(TOLS))
def test_fast_build_equals_the_plain_walk_build_and_the_oracle(tols, B, monkeypatch):
    fast = _check(tols, B, False, monkeypatch)
    sb = fast[6]
    assert sb[:, 12].min() > 0                              # the table index moved in every instance
    if tols == "coarse-forward":
        assert (sb[:, 0] > 4 * sb[:, 8]).all()              # several backward steps per stored point
    if tols == "coarse-backward":
        assert (sb[:, 8] > sb[:, 0]).all()                  # more stored points than backward steps: moves by two and more


def test_per_instance_times_launch_form(monkeypatch):
    _check("bench", 65, True, monkeypatch)
