"""Non-smooth right-hand sides on the device (pytest -m gpu): Abs, Max / Min, Piecewise, floor, Mod, sign, Heaviside.

Models and CPU-side pins: tests/test_nonsmooth.py (generated C against sympy at random points and ON every switching
surface; oracle against DOP853 truth across the kinks).  Here the device against the oracle BIT FOR BIT -- compared on
the uint64 view, so that -0.0 and +0.0 differ -- in every mapping a state-dependent select can take another route
through: one lane per instance, lean 4- and 8-lane groups (one family member per lane inside SA_FAM_BEGIN), 16 lanes and a
4-wavefront workgroup (one SA_SUM term per lane, SA_OWNS shares), the memory-resident kernel; both interpolations and
both record formats of the stored trajectory; both forward-sensitivity correctors.
"""
import functools

import numpy as np
import pytest

from tests.family_checks import CMP, CMP_B, TOL
from tests.helpers import make_oracle, make_problem
from tests.test_nonsmooth import KEYS, TRUTH_BARS, points
from tools.family_models import FAMILY
from tools.problems import kinked_batch

pytestmark = pytest.mark.gpu


def assert_same_bits(got, want, what=""):
    """Equal as bit patterns (NaN payloads aside: two NaNs count as equal); -0.0 != +0.0 here."""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    differ = (got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want))
    assert not differ.any(), (what, np.argwhere(differ)[:8].tolist(), got[differ][:8], want[differ][:8])


@functools.lru_cache(maxsize=None)
def _oracle_run(name, B, hermite=False):
    """Forward + adjoint of the B-draw batch in the oracle (computed once per model, batch size and interpolation)."""
    d = FAMILY[name].batch(B)
    orc = make_oracle(name)
    cfg = orc.config(rtol=1e-8, atol=1e-8, rtolB=1e-8, atolB=1e-8, rtolQB=1e-8, atolQB=1e-8, hermite=hermite)
    tv = d["tvals"]
    fwd = orc.solve_forward(cfg, d["y0"], d["ps"], d["pr"], 0.0, tv, nthreads=8)
    bwd = orc.solve_backward(cfg, tv[-1], 0.0, tv, d["grads"], nthreads=8)
    return d, fwd, bwd


def _device_equals_oracle(name, B, **solver_kw):
    from sunode_amd.solver import AdjointSolver
    d, (yo, so, sto), (go, lo, sbo, stbo) = _oracle_run(name, B, solver_kw.get("interpolation") == "hermite")
    tv = d["tvals"]
    sol = AdjointSolver(make_problem(name), **TOL, **solver_kw)
    y, st, stats = sol.solve_forward_batch(0.0, tv, d["y0"], d["ps"], d["pr"])
    g, lam, stb, statsb = sol.solve_backward_batch(tv[-1], 0.0, tv, d["grads"])
    sol._engine().close()
    assert (so == 0).all() and (sbo == 0).all()
    np.testing.assert_array_equal(st, so)
    np.testing.assert_array_equal(stb, sbo)
    np.testing.assert_array_equal(stats[:, CMP], sto[:, CMP])
    assert_same_bits(y, yo, "states")
    np.testing.assert_array_equal(statsb[:, CMP_B], stbo[:, CMP_B])
    assert_same_bits(g, go, "gradients")
    assert_same_bits(lam, lo, "lamda")
    return d, y, g, lam


def test_callbacks_equal_the_oracle_bitwise_on_every_surface():
    """``eval_callbacks`` of ``nonsmooth_fn`` at the points of tests/test_nonsmooth.py -- random, and ON every switching
    surface: equal arguments of Max / Min, x0 == a0 with a1 of either sign (a1 (x0 - a0) is -0 or +0 under Max(., 0)),
    t = 1, 2, 3/2, integers and -0 -- and at eight points with a NaN in one input (a NaN operand of Max / Min is ignored,
    of everything else it is not): all five callbacks and the return codes, bit for bit.

    This test decided how Max / Min are printed.  With the inherited ``fmax / fmin`` it failed at the point x0 == a0 =
    1.875, a1 = 1 (a1 (x0 - a0) = -0): output 1, ``fmin(x1, fmax(0.0, -0.0))``, was +0 on the device and -0 in the
    oracle, every other point agreeing.  Hence ``sa_max / sa_min`` (codegen.MINMAX_C): one rule on both sides."""
    from sunode_amd.solver import Solver
    prob = make_problem("nonsmooth_fn")
    eng = Solver(prob)._engine()
    orc = make_oracle("nonsmooth_fn")
    t, y, lam, ps, pr, n_random = points("nonsmooth_fn")
    t, y, lam, ps = (np.concatenate([v, v[n_random:n_random + 8]]) for v in (t, y, lam, ps))
    pr = np.zeros((len(t), 0))
    for k, (arr, col) in enumerate(((y, 1), (y, 2), (ps, 1), (y, 0), (ps, 0), (y, 3), (ps, 4), (ps, 2))):
        arr[len(t) - 8 + k, col] = np.nan
    with np.errstate(all="ignore"):
        got = eng.eval_callbacks(t, y, lam, ps, pr)
    n_zero = 0
    for i in range(len(t)):
        host = orc.eval(t[i], y[i], lam[i], ps[i], pr[i])
        for key in KEYS:
            assert_same_bits(got[key][i], host[key], "point %d (t=%r y=%r a=%r) %s" % (i, t[i], y[i], ps[i], key))
        assert got["codes"][i].tolist() == np.asarray(host["codes"]).tolist()
        if y[i, 0] == ps[i, 0] and np.isfinite(y[i]).all() and np.isfinite(ps[i]).all():
            n_zero += 1         # a1 (x0 - a0) is -0 or +0: sa_max(0.0, +-0) = +0 by the rule, whatever the order
            assert got["rhs"][i, 1] == 0.0 and not np.signbit(got["rhs"][i, 1])
    assert n_zero >= 3


@pytest.mark.parametrize("name", ["kinked", "threshold_sir4", "threshold_sir8", "threshold_sir16"])
def test_model_callbacks_equal_the_oracle_bitwise(name):
    """The integrated models' callbacks at their own surface points (I[j] == th and I[i] == 1 in some groups of an
    instance and not in others): the lane-family and SA_SUM forms of the generated text, bit for bit."""
    from sunode_amd.solver import Solver
    prob = make_problem(name)
    eng = Solver(prob)._engine()
    orc = make_oracle(name)
    t, y, lam, ps, pr, _ = points(name)
    got = eng.eval_callbacks(t, y, lam, ps, np.array([prob.extend_remainder(row) for row in pr]))
    for i in range(len(t)):
        host = orc.eval(t[i], y[i], lam[i], ps[i], pr[i])
        for key in KEYS:
            assert_same_bits(got[key][i], host[key], "point %d %s" % (i, key))
        assert got["codes"][i].tolist() == np.asarray(host["codes"]).tolist()


@pytest.mark.parametrize("group", [None] + list(FAMILY["kinked"].mappings))
def test_kinked_forward_adjoint_in_every_mapping(group, monkeypatch):
    """B = 37 (no multiple of a group size; draws cross the three surfaces at times spread over many steps, a fifth
    never reach one): statuses, every statistic, states, gradients and lamda equal the oracle's bit for bit."""
    if group:
        monkeypatch.setenv("SA_FORCE_GROUP", group)
    _device_equals_oracle("kinked", 37)


@pytest.mark.parametrize("kw", [dict(interpolation="hermite"), dict(compact_trajectory=False),
                                dict(compact_trajectory=True)], ids=["hermite", "table-records", "compact-records"])
def test_kinked_interpolation_and_record_formats(kw):
    """The stored trajectory across the kinks: Hermite interpolation, and both record formats of the polynomial one
    (table records; compact records, whose table the backward kernel rebuilds on every index move)."""
    _device_equals_oracle("kinked", 37, **kw)


def _against_truth(name, golden_dir):
    import os
    from sunode_amd.solver import AdjointSolver
    from tools.make_golden_truth import truth_errors
    d = np.load(os.path.join(golden_dir, "truth_%s.npz" % name))
    sol = AdjointSolver(make_problem(name), **TOL)
    tv = d["tvals"]
    y, st, _ = sol.solve_forward_batch(float(d["t0"]), tv, d["y0"], d["ps"], d["pr"])
    g, lam, stb, _ = sol.solve_backward_batch(tv[-1], float(d["t0"]), tv, d["grads"])
    assert (st == 0).all() and (stb == 0).all()
    err = truth_errors(dict(y_out=y, grad_params=g, grad_y0=-lam), d)
    print(name, "device against truth:", err)
    for key in ("y", "grad_params", "grad_y0"):
        assert err[key] <= TRUTH_BARS[name][key], (key, err[key])


def test_kinked_matches_truth(golden_dir):
    """Device against DOP853 truth (tests/golden/truth_kinked.npz) at the bars of tests/test_nonsmooth.py."""
    _against_truth("kinked", golden_dir)


@pytest.mark.parametrize("M,group", [(M, group) for M in (4, 8, 16)
                                     for group in [None] + list(FAMILY["threshold_sir%d" % M].mappings)])
def test_threshold_sir_lanes_on_different_branches(M, group, monkeypatch):
    """B = 21; in every instance some groups start above the threshold and some below (and above / below the saturation
    level of the recovery): lanes of one instance are on different branches inside SA_FAM_BEGIN (M = 4: lean 4-lane
    groups, 8 lanes; M = 8: lean groups, workgroup) and inside SA_SUM terms (M = 16: 16 lanes, workgroup, memory).
    ``None`` is the engine's own mapping of the model (batch_mapping="fixed": no small-batch substitute)."""
    if group:
        monkeypatch.setenv("SA_FORCE_GROUP", group)
    d, y, _, _ = _device_equals_oracle("threshold_sir%d" % M, 21, batch_mapping="fixed")
    th = d["ps"][:, -1:]
    above0 = (d["y0"][:, M:] > th).sum(axis=1)
    assert ((above0 > 0) & (above0 < M)).all()
    above = (y[:, :, M:] > th[:, None, :]).sum(axis=2)              # at every output time
    assert ((above > 0) & (above < M)).any(axis=1).all()
    assert ((y[:, :, M:] > 1.0).any(axis=(1, 2)) & (y[:, :, M:] < 1.0).any(axis=(1, 2))).all()


def test_threshold_sir8_matches_truth(golden_dir):
    _against_truth("threshold_sir8", golden_dir)


@pytest.mark.parametrize("mode", ["simultaneous", "staggered"])
def test_kinked_forward_sensitivities(mode):
    """``Solver(sens_mode=...)`` at B = 16: states, sensitivities and statistics equal the oracle's bit for bit."""
    from sunode_amd.solver import Solver
    prob = make_problem("kinked")
    d = kinked_batch(16)
    tv = d["tvals"]
    sol = Solver(prob, abstol=1e-8, reltol=1e-8, sens_mode=mode)
    sens0 = np.zeros((prob.n_params, prob.n_states))
    y, sens, st, stats = sol.solve_sens_batch(0.0, tv, d["y0"], d["ps"], d["pr"], sens0)
    orc = make_oracle("kinked")
    yo, seno, so, sto = orc.solve_sens(orc.config(rtol=1e-8, atol=1e-8), d["y0"], d["ps"], d["pr"], sens0, 0.0, tv,
                                       mode=mode, nthreads=8)
    assert (st == 0).all() and (so == 0).all()
    assert_same_bits(y, yo, "states")
    assert_same_bits(sens, seno, "sensitivities")
    np.testing.assert_array_equal(stats[:, CMP[:8]], sto[:, CMP[:8]])


def test_nan_initial_states_fail_like_the_oracle():
    """A NaN initial state in 3 of 16 instances (x, y or z: Max(y - th, 0) swallows a NaN y on its way into x', the
    other terms do not): per-instance statuses equal the oracle's and every other instance equals it bit for bit.  Pins
    that both sides agree, not which status is right."""
    from sunode_amd.solver import AdjointSolver
    prob = make_problem("kinked")
    d = kinked_batch(16)
    y0 = d["y0"].copy()
    y0[2, 1] = y0[7, 0] = y0[11, 2] = np.nan
    sol = AdjointSolver(prob, **TOL)
    y, st, stats = sol.solve_forward_batch(0.0, d["tvals"], y0, d["ps"], d["pr"])
    orc = make_oracle("kinked")
    cfg = orc.config(rtol=1e-8, atol=1e-8, rtolB=1e-8, atolB=1e-8, rtolQB=1e-8, atolQB=1e-8)
    yo, so, sto = orc.solve_forward(cfg, y0, d["ps"], d["pr"], 0.0, d["tvals"], nthreads=8)
    np.testing.assert_array_equal(st, so)
    ok = np.ones(16, bool)
    ok[[2, 7, 11]] = False
    assert (so[ok] == 0).all() and (so[~ok] != 0).all()
    assert_same_bits(y[ok], yo[ok], "states of the other instances")
    np.testing.assert_array_equal(stats[ok][:, CMP], sto[ok][:, CMP])
