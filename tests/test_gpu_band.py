"""``linear_solver="band"`` on the device (pytest -m gpu): the band build of the memory-resident mapping against the CPU
oracle and against the dense memory-resident build, bit for bit.

The oracle factors the dense matrix.  A partial-pivoting LU of a matrix whose entries outside the band are exact zeros
performs the dense LU's floating-point operations on the entries inside it, in the same order (csrc/bdf_mem.hip,
tests/test_band.py), so states, gradients, statuses and step counters must be ``array_equal`` -- rtol = atol = 1e-8 and
B = 21 unless noted; small models reach the mapping through SA_FORCE_GROUP=mem."""
import functools

import numpy as np
import pytest

from sunode_amd import _native
from tests.helpers import make_oracle, make_problem
from tools.problems import brusselator1d_batch, chain_batch

pytestmark = pytest.mark.gpu

CMP = [0, 1, 2, 3, 4, 5, 6, 7, 8]            # as tests/test_gpu_parity.py: the counters the oracle keeps
CMP_B = [0, 1, 2, 3, 4, 5, 6, 9, 10, 12]
B = 21


def _tol(rtol=1e-8, atol=1e-8):
    return dict(abstol=atol, reltol=rtol, backward_abstol=atol, backward_reltol=rtol, quad_abstol=atol, quad_reltol=rtol)


def _band_kw(ml, mu):
    return dict(linear_solver="band", linear_solver_kwargs={"lower_bandwidth": ml, "upper_bandwidth": mu})


def _adjoint(sol, d):
    """forward + backward of one batch: y, status, stats, grad, lamda_out, status_b, stats_b"""
    tv = d["tvals"]
    y, st, sc = sol.solve_forward_batch(d["t0"], tv, d["y0"], d["ps"], d["pr"])
    g, lam, stb, scb = sol.solve_backward_batch(tv[-1], d["t0"], tv, d["grads"])
    return [np.array(a) for a in (y, st, sc, g, lam, stb, scb)]


def _oracle_adjoint(name, d, hermite=False, rtol=1e-8, atol=1e-8):
    orc = make_oracle(name)
    cfg = orc.config(rtol=rtol, atol=atol, rtolB=rtol, atolB=atol, rtolQB=rtol, atolQB=atol, hermite=hermite)
    tv = d["tvals"]
    y, st, sc = orc.solve_forward(cfg, d["y0"], d["ps"], d["pr"], d["t0"], tv, nthreads=8)
    g, lam, stb, scb = orc.solve_backward(cfg, tv[-1], d["t0"], tv, d["grads"], nthreads=8)
    return [y, st, sc, g[:, :d["ps"].shape[1]], lam, stb, scb]


def _assert_same(got, want, oracle=True):
    """``oracle``: the counters the oracle keeps; otherwise (two device builds) all of them."""
    assert (want[1] == 0).all() and (want[5] == 0).all()
    for k, (x, y) in enumerate(zip(got, want)):
        if oracle and k in (2, 6):
            cols = CMP if k == 2 else CMP_B
            x, y = x[:, cols], y[:, cols]
        np.testing.assert_array_equal(x, y, err_msg="output %d" % k)


@functools.lru_cache(maxsize=None)
def _brusselator6(hermite):
    """(batch, oracle result, dense memory-resident result) of brusselator1d(6), computed once"""
    import os
    from sunode_amd.solver import AdjointSolver
    assert os.environ.get("SA_FORCE_GROUP") == "mem"
    d = brusselator1d_batch(B, 6)
    interp = "hermite" if hermite else "polynomial"
    dense = _adjoint(AdjointSolver(make_problem("brusselator1d_6"), interpolation=interp, **_tol()), d)
    want = _oracle_adjoint("brusselator1d_6", d, hermite=hermite)
    for a in dense + want:
        a.setflags(write=False)
    return d, want, dense


@pytest.mark.parametrize("ml, mu, hermite", [(2, 2, False), (3, 4, False), (2, 2, True)],
                         ids=["exact", "over-declared", "hermite"])
def test_brusselator_band_equals_oracle_and_dense_build(ml, mu, hermite, monkeypatch):
    from sunode_amd.solver import AdjointSolver
    monkeypatch.setenv("SA_FORCE_GROUP", "mem")
    d, want, dense = _brusselator6(hermite)
    sol = AdjointSolver(make_problem("brusselator1d_6"), interpolation="hermite" if hermite else "polynomial",
                        **_tol(), **_band_kw(ml, mu))
    eng = sol._engine()
    assert eng.variant == ("bdf_mem.hip", 1)
    assert eng.code_object == _native.code_object_path(sol._source, hermite=hermite, band=(ml, mu))
    got = _adjoint(sol, d)
    assert got[2][:, 3].min() >= 2 and got[2][:, 2].min() > got[2][:, 3].max()      # fresh AND restored Jacobians
    _assert_same(got, want)
    _assert_same(got, dense, oracle=False)


def test_brusselator_band_with_the_guard_on(monkeypatch):
    """The product configuration: the band build and its conservative partner (same band defines) compared on the device."""
    from sunode_amd.solver import AdjointSolver
    monkeypatch.setenv("SA_FORCE_GROUP", "mem")
    d, want, _ = _brusselator6(False)           # (the dense build's run: before the guard is switched on)
    monkeypatch.setenv("SA_GUARD", "1")
    sol = AdjointSolver(make_problem("brusselator1d_6"), **_tol(), **_band_kw(2, 2))
    eng = sol._engine()
    assert eng.guard_report["enabled"]
    assert eng.guard_report["conservative"] in _native.code_object_path(sol._source, band=(2, 2), safe=True)
    got = _adjoint(sol, d)
    state = eng.guard_state()
    assert "adjoint" in state["verified"] and not state["differs"] and not state["using_conservative"], state
    _assert_same(got, want)


@pytest.mark.parametrize("name, ml, mu", [("pivoting_band", 1, 1), ("pivoting", 5, 1)], ids=["tridiagonal", "nearly-full"])
def test_row_exchanges_in_the_band_lu(name, ml, mu, monkeypatch):
    """The inputs of tests/test_gpu_parity.py::test_row_exchanges_in_the_dense_lu: rotations at 1000 rad/s far below
    the tolerances, steps of order 1 -- the LU exchanges rows in the forward and in the backward solve, inside the band
    (fill-in above it) and in a band that covers nearly all of the matrix (the lower width at its clamp, n - 1 = 5)."""
    from sunode_amd.solver import AdjointSolver
    monkeypatch.setenv("SA_FORCE_GROUP", "mem")
    prob = make_problem(name)
    rng = np.random.RandomState(0)
    d = dict(ps=np.array([0.5, 0.3]) * np.exp(0.1 * rng.randn(B, 2)), pr=np.array([1000.0, 700.0]),
             y0=np.tile([0.5, 1e-6, 0.0, 1e-6, 2e-6, 0.1], (B, 1)), tvals=np.linspace(0, 20, 11), t0=0.0)
    d["grads"] = np.ones((11, 6))
    d["grads"][:, 1:5] = 0.0
    sol = AdjointSolver(prob, **_tol(1e-5, 1e-4), **_band_kw(ml, mu))
    assert sol._engine_kwargs()["band"] == (min(ml, 5), min(mu, 5))
    got = _adjoint(sol, d)
    assert got[2][:, 0].max() < 80                      # steps of order 0.5: gamma * omega >> 1, rows get exchanged
    _assert_same(got, _oracle_adjoint(name, d, rtol=1e-5, atol=1e-4))


def test_solver_band_plain_and_sensitivities(monkeypatch):
    """``Solver``: plain solves and both sensitivity correctors through the band LU (brusselator1d(3), n = 6, p = 2), and
    per-instance t0 [B] / tvals [B, n_t] once."""
    from sunode_amd.solver import Solver, initial_sensitivities
    monkeypatch.setenv("SA_FORCE_GROUP", "mem")
    prob = make_problem("brusselator1d_3")
    d = brusselator1d_batch(B, 3)
    orc = make_oracle("brusselator1d_3")
    cfg = orc.config(rtol=1e-8, atol=1e-8)
    tv = d["tvals"]
    sol = Solver(prob, abstol=1e-8, reltol=1e-8, **_band_kw(2, 2))
    assert sol._engine().code_object == _native.code_object_path(sol._source, band=(2, 2))
    y, st, sc = sol.solve_batch(0.0, tv, d["y0"], d["ps"], d["pr"])
    yo, so, sco = orc.solve(cfg, d["y0"], d["ps"], d["pr"], 0.0, tv, nthreads=8)
    assert (so == 0).all()
    np.testing.assert_array_equal(st, so)
    np.testing.assert_array_equal(sc[:, CMP[:8]], sco[:, CMP[:8]])
    np.testing.assert_array_equal(y, yo)
    # every instance with its own start time and grid = the oracle called per instance
    rng = np.random.default_rng(7)
    t0 = rng.uniform(0.0, 0.3, B)
    tvs = np.sort(t0[:, None] + rng.uniform(0.0, 2.0, (B, 4)), axis=1)
    y, st, sc = sol.solve_batch(t0, tvs, d["y0"], d["ps"], d["pr"])
    want = [orc.solve(cfg, d["y0"][b:b + 1], d["ps"][b:b + 1], d["pr"], float(t0[b]), tvs[b]) for b in range(B)]
    assert all((w[1] == 0).all() for w in want)
    np.testing.assert_array_equal(st, np.concatenate([w[1] for w in want]))
    np.testing.assert_array_equal(sc[:, CMP[:8]], np.concatenate([w[2] for w in want])[:, CMP[:8]])
    np.testing.assert_array_equal(y, np.concatenate([w[0] for w in want]))
    sens0 = initial_sensitivities(prob)
    for mode in ("simultaneous", "staggered"):
        ssol = Solver(prob, abstol=1e-8, reltol=1e-8, sens_mode=mode, **_band_kw(2, 2))
        assert ssol._engine().code_object == _native.code_object_path(ssol._source, sens=True, band=(2, 2))
        y, s, st, sc = ssol.solve_sens_batch(0.0, tv, d["y0"], d["ps"], d["pr"], sens0)
        yo, so_, sto, sco = orc.solve_sens(cfg, d["y0"], d["ps"], d["pr"], sens0, 0.0, tv, mode=mode, nthreads=8)
        assert (sto == 0).all()
        np.testing.assert_array_equal(st, sto)
        np.testing.assert_array_equal(sc[:, CMP[:8]], sco[:, CMP[:8]])
        np.testing.assert_array_equal(y, yo)
        np.testing.assert_array_equal(s, so_)


@pytest.mark.parametrize("name, batch, ml, mu", [("chain256", 24, 1, 0), ("brusselator1d_65", 8, 2, 2)])
def test_band_on_the_natural_path(name, batch, ml, mu, monkeypatch):
    """More than 128 states: the engine selects the memory-resident mapping by itself and the band is honoured.  The
    workspace the band code object announces is the band formula's and far smaller than the dense one's."""
    from sunode_amd.solver import AdjointSolver
    monkeypatch.delenv("SA_FORCE_GROUP", raising=False)
    prob = make_problem(name)
    n = prob.n_states
    d = chain_batch(batch, n) if name.startswith("chain") else brusselator1d_batch(batch, n // 2)
    d = dict(d, rtol=1e-8, atol=1e-8)
    sol = AdjointSolver(prob, **_tol(d["rtol"], d["atol"]), **_band_kw(ml, mu))
    eng = sol._engine()
    assert eng.variant == ("bdf_mem.hip", 1)
    ws = _native.code_object_meta(eng.code_object)["ws_doubles"]
    # csrc/bdf_mem.hip O_*: 43 state-sized and 17 parameter-sized vectors and the norm's tree next to the matrices, which
    # are 2 n^2 in the dense build and, here, O_A (2 max + min + 1) n -- one place for the forward problem's
    # (2 ml + mu + 1) n and the backward problem's swapped widths -- and O_SJ (ml + mu + 1) n
    p = prob.n_params
    vectors = 43 * n + 17 * p + (1 << (max(n, p) - 1).bit_length())
    band_part = (2 * max(ml, mu) + min(ml, mu) + 1) * n + (ml + mu + 1) * n
    assert ws == vectors + band_part < vectors + 2 * n * n
    if name == "chain256":          # (the dense build of the sweep is there to be asked)
        assert _native.code_object_meta(_native.code_object_path(sol._source))["ws_doubles"] == vectors + 2 * n * n
    got = _adjoint(sol, d)
    _assert_same(got, _oracle_adjoint(name, d, rtol=d["rtol"], atol=d["atol"]))
