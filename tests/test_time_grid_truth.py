"""Per-instance start times, output grids and backward end times against a truth that does not share the callbacks.

tests/golden/truth_times_<name>.npz (tools/make_golden_truth.py --times: DOP853 at rtol 1e-13 on the model augmented
with its sensitivity equations) holds t0 [B], tvals [B, n_t], tend [B] on the two models whose right-hand side reads t
-- ``forcing`` (B-spline input, expit(k (t - t_mid))) and ``misc`` (sin t) -- with the edge rows the generator's
docstring lists: windows across the spline's support edge, t0 ~ 1e3 and ~ 1e5, tvals[b, 0] == t0[b], repeated output
times, spans 10^3 apart, tend strictly between t0 and tvals[b, 0], and n_t = 1 (keys ``one_*``).

Here the CPU oracle, called per instance, is held to the suite's bars at rtol = atol = 1e-8: states <= 1e-5 of the
largest |y| of each component, gradients and dL/dy(tend) <= 4e-6 relative per instance, forward sensitivities <= 2e-5
of the largest |dy/dp| of the instance.  tests/test_gpu_time_grid_truth.py holds the device to the oracle's bits and
to the same bars."""
import os

import numpy as np
import pytest

from tests.helpers import make_oracle, make_problem

MODELS = ["forcing", "misc"]
TOL = 1e-8


def load_truth(golden_dir, name, one=False):
    """The fixture's arrays; ``one``: the n_t = 1 rows under the plain names."""
    t = np.load(os.path.join(golden_dir, "truth_times_%s.npz" % name))
    d = {k: t[k] for k in t.files if not k.startswith("one_")}
    if one:
        d.update({k[4:]: t[k] for k in t.files if k.startswith("one_")})
        d["y0"], d["ps"] = d["y0"][:len(d["t0"])], d["ps"][:len(d["t0"])]
    return d


def check_truth(t, y=None, g=None, lam=None, sens=None):
    """The suite's bars against the truth fixture ``t`` (rows in the fixture's order)."""
    if y is not None:
        err = np.abs(y - t["y_out"]) / np.abs(t["y_out"]).max(axis=(0, 1))
        assert err.max() < 1e-5, ("states", np.unravel_index(err.argmax(), err.shape), err.max())
    for got, key in ((g, "grad_params"), (None if lam is None else -lam, "grad_y_tend")):
        if got is not None:
            err = np.abs(got - t[key]) / np.abs(t[key]).max(axis=1, keepdims=True)
            assert err.max() < 4e-6, (key, np.unravel_index(err.argmax(), err.shape), err.max())
    if sens is not None:
        err = np.abs(sens - t["sens"]) / np.abs(t["sens"]).max(axis=(1, 2, 3), keepdims=True)
        assert err.max() < 2e-5, ("sensitivities", np.unravel_index(err.argmax(), err.shape), err.max())


def no_forward(t):
    """Rows whose forward pass takes no step (every output time at t0): no trajectory, so the backward pass reports
    CV_NO_FWD (-102) with NaN outputs -- the oracle's and the device's semantics alike."""
    return t["tvals"][:, -1] == t["t0"]


def check_adjoint_truth(t, y, st, g, lam, stb):
    """Statuses (0, or CV_NO_FWD on the ``no_forward`` rows) and the truth bars on the rows that integrate."""
    nf = no_forward(t)
    assert (st == 0).all() and (stb[~nf] == 0).all() and (stb[nf] == -102).all(), (st, stb)
    assert np.isnan(g[nf]).all() and np.isnan(lam[nf]).all()
    check_truth(t, y=y)
    check_truth({k: t[k][~nf] for k in ("grad_params", "grad_y_tend")}, g=g[~nf], lam=lam[~nf])


def oracle_config(orc, hermite=False):
    return orc.config(rtol=TOL, atol=TOL, rtolB=TOL, atolB=TOL, rtolQB=TOL, atolQB=TOL, hermite=hermite)


def oracle_adjoint(name, t, hermite=False):
    """The oracle instance by instance with its own t0 / tvals / tend: y, status, stats, g, lam, status_b, stats_b,
    lamda_all, quad_all."""
    orc = make_oracle(name)
    cfg = oracle_config(orc, hermite)
    pr = t["pr"]
    rows = []
    for b in range(len(t["t0"])):
        prb = pr[b:b + 1] if pr.ndim == 2 else pr
        tv = t["tvals"][b]
        y, st, sc = orc.solve_forward(cfg, t["y0"][b:b + 1], t["ps"][b:b + 1], prb, float(t["t0"][b]), tv)
        g, lam, stb, scb, la, qa = orc.solve_backward(cfg, tv[-1], float(t["tend"][b]), tv, t["grads"][b:b + 1],
                                                      return_all=True)
        rows.append((y, st, sc, g, lam, stb, scb, la, qa))
    return [np.concatenate(c) for c in zip(*rows)]


def oracle_sens(name, t, mode):
    """Solver(sens_mode=mode) on the oracle per instance from t0 with initial_sensitivities: y, sens, status, stats."""
    from sunode_amd.solver import initial_sensitivities
    orc = make_oracle(name)
    cfg = orc.config(rtol=TOL, atol=TOL)
    sens0 = initial_sensitivities(make_problem(name))
    pr = t["pr"]
    rows = [orc.solve_sens(cfg, t["y0"][b:b + 1], t["ps"][b:b + 1], pr[b:b + 1] if pr.ndim == 2 else pr, sens0[None],
                           float(t["t0"][b]), t["tvals"][b], mode=mode) for b in range(len(t["t0"]))]
    return [np.concatenate(c) for c in zip(*rows)]


def test_fixture_rows_cover_the_edges(golden_dir):
    """The rows the fixtures promise (a regenerated fixture that lost one would stop testing it)."""
    for name in MODELS:
        t = load_truth(golden_dir, name)
        t0, tv, tend = t["t0"], t["tvals"], t["tend"]
        assert (tv[:, 0] == t0).any() and (tv[:, 1] == t0).any()             # first output at t0, t0 repeated
        assert (np.diff(tv, axis=1) == 0).any(axis=1).sum() >= 8               # repeated output times
        inner = (tend > t0) & (tend < tv[:, 0])
        assert inner.sum() >= 4 and (tend[~inner] == t0[~inner]).all()
        span = tv[:, -1] - t0
        assert span.max() / span.min() > 500
        one = load_truth(golden_dir, name, one=True)
        assert one["tvals"].shape[1] == 1 and no_forward(one).sum() == 1 and (one["tend"] > one["t0"]).any()
        assert not no_forward(t).any()
    f, m = load_truth(golden_dir, "forcing"), load_truth(golden_dir, "misc")
    assert (f["t0"] < 0).sum() >= 4 and ((f["t0"] < 0) & (f["tvals"][:, -1] > 0)).any()       # across the spline's edge
    assert (np.abs(m["t0"] - 1e3) < 10).sum() >= 4 and (np.abs(m["t0"] - 1e5) < 10).sum() >= 4


@pytest.mark.parametrize("one", [False, True], ids=["grid", "n_t1"])
@pytest.mark.parametrize("name", MODELS)
def test_oracle_adjoint_per_instance_times_vs_truth(name, one, golden_dir):
    t = load_truth(golden_dir, name, one)
    y, st, _, g, lam, stb, _, _, _ = oracle_adjoint(name, t)
    check_adjoint_truth(t, y, st, g, lam, stb)


@pytest.mark.parametrize("mode", ["simultaneous", "staggered"])
@pytest.mark.parametrize("name", MODELS)
def test_oracle_sensitivities_per_instance_times_vs_truth(name, mode, golden_dir):
    t = load_truth(golden_dir, name)
    y, sens, st, _ = oracle_sens(name, t, mode)
    assert (st == 0).all(), st
    check_truth(t, y=y, sens=sens)


@pytest.mark.parametrize("name", MODELS)
def test_oracle_hermite_per_instance_times_vs_truth(name, golden_dir):
    t = load_truth(golden_dir, name)
    y, st, _, g, lam, stb, _, _, _ = oracle_adjoint(name, t, hermite=True)
    check_adjoint_truth(t, y, st, g, lam, stb)
