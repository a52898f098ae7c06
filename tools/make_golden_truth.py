"""Generate tests/golden/truth_*.npz and tests/golden/dvode_stats.json.

Independent oracles for the integrator half:

* ``dvode_stats.json``: scipy.integrate.ode('vode', method='bdf') -- Fortran DVODE, the
  direct ancestor of CVODE -- step statistics and end states on Lotka-Volterra /
  Robertson.  The CVODE forward controller reproduces these counters exactly on LV.
* ``truth_<name>.npz``: tight-tolerance solutions (DOP853 / Radau, rtol 1e-13) of
  the ODE *augmented with its forward sensitivity equations* dS/dt = J S + df/dp
  (and dS0/dt = J S0 for the initial-value sensitivities), giving y(t_k) and the
  exact gradients of L = sum_k sum_i g[k,i] y_i(t_k) w.r.t. the differentiated
  parameters and y0 -- what ``solve_backward`` returns as ``grad_out`` and
  ``-lamda_out`` (/root/reference/sunode/solver.py:783-784,
  wrappers/as_pytensor.py:294-308).

Usage: python tools/make_golden_truth.py   (a few minutes; outputs are committed)
       python tools/make_golden_truth.py --times    (only truth_times_<name>.npz: see ``times_truth``)
       python tools/make_golden_truth.py --transcendental | --inverse-erf | --gamma | --bessel | --prob
                                                    (only the fixtures of that family: see ``FAMILY_FLAGS``, ``family_truth``)
       python tools/make_golden_truth.py --nonsmooth    (only truth_kinked.npz, truth_threshold_sir8.npz: see ``nonsmooth_truth``)
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import sympy as sym
from scipy.integrate import ode, solve_ivp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from sunode_amd import SympyProblem  # noqa: E402
from sunode_amd.symode.problem import HOST_FUNCTIONS, host_form  # noqa: E402
from tools.family_models import FAMILY  # noqa: E402
from tools.problems import (EXTRA_PROBLEMS, PROBLEMS, _cotangents, forcing_batch, lv_batch, misc_batch,  # noqa: E402
                            robertson_batch, seir_batch)

GOLD = os.path.join(ROOT, "tests", "golden")


def make(name):
    s = {**PROBLEMS, **EXTRA_PROBLEMS}[name]
    return SympyProblem(s["params"], s["states"], s["rhs"], s["derivative_params"])


def augmented_rhs(prob):
    """Callable f(t, z, ps, pr) for z = [y, S (n x p, column-major by param), S0 (n x n)]."""
    n, p = prob.n_states, prob.n_params
    y = list(prob._sym_statevec)
    ps = list(prob._sym_deriv_paramsvec)
    pr = list(prob._sym_fixed_paramsvec)
    f = sym.lambdify([prob._sym_time, y, ps, pr], [host_form(e) for e in prob._sym_dydt], modules=[HOST_FUNCTIONS, "numpy"], cse=True)
    J = sym.lambdify([prob._sym_time, y, ps, pr], sym.Matrix(prob._sym_dydt_jac).applyfunc(host_form), modules=[HOST_FUNCTIONS, "numpy"], cse=True)
    P = sym.lambdify([prob._sym_time, y, ps, pr], sym.Matrix(prob._sym_dydp).applyfunc(host_form), modules=[HOST_FUNCTIONS, "numpy"], cse=True) if p else None

    def rhs(t, z, psv, prv):
        yv = z[:n]
        S = z[n:n + n * p].reshape(p, n).T
        S0 = z[n + n * p:].reshape(n, n).T
        Jv = np.asarray(J(t, yv, psv, prv), dtype=float).reshape(n, n)
        out = np.empty_like(z)
        out[:n] = np.asarray(f(t, yv, psv, prv), dtype=float)
        if p:
            Pv = np.asarray(P(t, yv, psv, prv), dtype=float).reshape(n, p)
            out[n:n + n * p] = (Jv @ S + Pv).T.ravel()
        out[n + n * p:] = (Jv @ S0).T.ravel()
        return out
    return rhs


def truth_batch(prob, y0, ps, pr, t0, tvals, grads, method, rtol=1e-13, atol=1e-15, return_sens=False):
    """-> y_out [B, n_t, n], dL/dp [B, p], dL/dy0 [B, n] (and, ``return_sens``, the forward sensitivities
    [B, n_t, p, n] they were contracted from)."""
    n, p = prob.n_states, prob.n_params
    B = y0.shape[0]
    rhs = augmented_rhs(prob)
    y_out = np.zeros((B, len(tvals), n))
    grad_p = np.zeros((B, p))
    grad_y0 = np.zeros((B, n))
    sens = np.zeros((B, len(tvals), p, n))
    for b in range(B):
        prb = pr if pr.ndim == 1 else pr[b]
        z0 = np.concatenate([y0[b], np.zeros(n * p), np.eye(n).ravel()])
        sol = solve_ivp(rhs, (t0, tvals[-1]), z0, method=method, t_eval=tvals, args=(ps[b], prb),
                        rtol=rtol, atol=atol)
        assert sol.success, sol.message
        z = sol.y.T
        y_out[b] = z[:, :n]
        g = grads if grads.ndim == 2 else grads[b]
        S = z[:, n:n + n * p].reshape(len(tvals), p, n)
        S0 = z[:, n + n * p:].reshape(len(tvals), n, n)        # [k, j(y0 index), i(state)]
        grad_p[b] = np.einsum("ki,kpi->p", g, S)
        grad_y0[b] = np.einsum("ki,kji->j", g, S0)
        sens[b] = S
        print("  truth instance", b, "nfev", sol.nfev, flush=True)
    if return_sens:
        return y_out, grad_p, grad_y0, sens
    return y_out, grad_p, grad_y0


def cotangent(n_t, n):
    """Non-degenerate dL/dy_out: Robertson and SEIR conserve sum(y), so grads = ones
    (BASELINE's loss = sum(y_out)) has an identically-zero parameter gradient there."""
    k = np.arange(n_t)[:, None]
    i = np.arange(n)[None, :]
    return 1.0 + 0.5 * np.cos(1.7 * k + 0.9 * i)


def dvode_run(f, jac, y0, tvals, rtol, atol, args):
    r = ode(f, jac).set_integrator("vode", method="bdf", with_jacobian=True, rtol=rtol, atol=atol, nsteps=100000)
    r.set_initial_value(y0, tvals[0]).set_f_params(*args).set_jac_params(*args)
    ys = [np.array(y0, float)]
    for t in tvals[1:]:
        ys.append(r.integrate(t).copy())
        assert r.successful()
    iw = r._integrator.iwork
    return dict(nst=int(iw[10]), nfe=int(iw[11]), nje=int(iw[12]), qlast=int(iw[13]), nlu=int(iw[18]),
                nni=int(iw[19]), ncfn=int(iw[20]), netf=int(iw[21]), y=np.array(ys).tolist())


def family_truth(name):
    """truth_<name>.npz of an integrated model of a smooth function family (tools/family_models.py: its batch and number
    of draws, per-instance cotangents).  Nothing of csrc/sa_math*.h is on this side: the host functions are numpy's and
    scipy.special's (erf / erfc; gammaln / gamma / digamma / polygamma; jv / yv / iv / kv; erfinv / erfcinv / gammainc / gammaincc), and the B-spline of ``forcing``
    is evaluated by the Cox-de Boor recursion, NOT by the polynomial pieces the generated code shares with the
    reference."""
    prob = make(name)
    d = FAMILY[name].batch(FAMILY[name].truth_draws)
    y_out, gp, gy0 = truth_batch(prob, d["y0"], d["ps"], d["pr"], d["t0"], d["tvals"], d["grads"], "DOP853")
    np.savez(os.path.join(GOLD, "truth_%s.npz" % name), y0=d["y0"], ps=d["ps"], pr=d["pr"], t0=d["t0"],
             tvals=d["tvals"], grads=d["grads"], y_out=y_out, grad_params=gp, grad_y0=gy0)


#: command-line flag -> the models whose truth ``family_truth`` writes
FAMILY_FLAGS = {"--transcendental": ("forcing", "logistic_switch", "misc"), "--inverse-erf": ("probit_gate",),
                "--gamma": ("gamma_delay",), "--bessel": ("bessel_ring",), "--prob": ("quantile_delay",)}


#: what the two DOP853 runs of ``nonsmooth_truth`` (rtol 1e-13 and 1e-11) must agree to, in the tests' own error
#: measures: a hundredth of the bars of tests/test_nonsmooth.py (TRUTH_BARS there; the test re-checks the stored figures)
NONSMOOTH_AGREE = {"kinked": dict(y=6.9e-9, grad_params=9.1e-9, grad_y0=8.6e-9, sens=4.3e-8),
                   "threshold_sir8": dict(y=1.3e-8, grad_params=3.1e-8, grad_y0=4.6e-8)}


def truth_errors(got, ref):
    """{quantity: error of ``got`` against ``ref``} in the measures of the truth tests: states relative to the largest
    value of the component over the batch, gradients relative to the largest component of the draw's gradient,
    sensitivities relative to the largest value of the (parameter, state) pair over the batch."""
    out = {"y": float(np.max(np.abs(got["y_out"] - ref["y_out"]) / np.abs(ref["y_out"]).max(axis=(0, 1))))}
    for key, short in (("grad_params", "grad_params"), ("grad_y0", "grad_y0")):
        out[short] = float(np.max(np.abs(got[key] - ref[key]) / np.abs(ref[key]).max(axis=1, keepdims=True)))
    if "sens" in got and "sens" in ref:
        scale = np.abs(ref["sens"]).max(axis=(0, 1))
        out["sens"] = float(np.max(np.abs(got["sens"] - ref["sens"]) / np.where(scale > 0, scale, 1.0)))
    return out


def nonsmooth_truth():
    """truth_kinked.npz, truth_threshold_sir8.npz: 8 draws each of the models with a continuous but kinked right-hand
    side (Max / Abs / Piecewise of a state; numpy's amax / abs / select / heaviside / sign on this side).  A one-step
    method's error estimate across a kink is not a given, so every fixture is integrated twice -- DOP853 at rtol 1e-13
    (stored) and at 1e-11 -- and the two must agree to ``NONSMOOTH_AGREE``, a hundredth of the bars the tests apply; the
    measured agreement is stored next to the truth (``agree_<quantity>``).  ``kinked`` also stores the forward
    sensitivities dy/dp [B, n_t, p, n]."""
    for name in ("kinked", "threshold_sir8"):
        prob = make(name)
        d = FAMILY[name].batch(FAMILY[name].truth_draws)
        runs = []
        for rtol, atol in ((1e-13, 1e-15), (1e-11, 1e-13)):
            y_out, gp, gy0, sens = truth_batch(prob, d["y0"], d["ps"], d["pr"], d["t0"], d["tvals"], d["grads"], "DOP853",
                                               rtol=rtol, atol=atol, return_sens=True)
            runs.append(dict(y_out=y_out, grad_params=gp, grad_y0=gy0, sens=sens))
        agree = truth_errors(runs[1], runs[0])
        print(name, "DOP853 1e-11 against 1e-13:", agree, flush=True)
        for key, bound in NONSMOOTH_AGREE[name].items():
            assert agree[key] <= bound, (name, key, agree[key], bound)
        extra = {"sens": runs[0]["sens"]} if name == "kinked" else {}
        np.savez(os.path.join(GOLD, "truth_%s.npz" % name), y0=d["y0"], ps=d["ps"], pr=d["pr"], t0=d["t0"],
                 tvals=d["tvals"], grads=d["grads"], y_out=runs[0]["y_out"], grad_params=runs[0]["grad_params"],
                 grad_y0=runs[0]["grad_y0"], **extra, **{"agree_" + k: v for k, v in agree.items()})


def sweep_truth():
    """truth_sweep_<name>.npz for every shape of the parity sweep (tests/test_shape_sweep.py, tests/test_sweep_truth.py):
    4 draws each of the sweep's own batch -- from the hand-written closed form of the sweep's model families, not from
    this module's lambdified ``prob._sym_*`` (tools/make_golden_truth_sweep.py; ``truth_batch`` here stays the second,
    symbolic derivation the tests compare it with on ``lv12`` and ``rn12_4``)."""
    from tools import make_golden_truth_sweep
    make_golden_truth_sweep.main()


def plain_rhs(prob):
    """Callable f(t, y, ps, pr) -> dy/dt of the model alone."""
    y = list(prob._sym_statevec)
    f = sym.lambdify([prob._sym_time, y, list(prob._sym_deriv_paramsvec), list(prob._sym_fixed_paramsvec)],
                     list(prob._sym_dydt), modules=[HOST_FUNCTIONS, "numpy"], cse=True)
    return lambda t, yv, psv, prv: np.asarray(f(t, yv, psv, prv), dtype=float)


def truth_times_batch(prob, y0, ps, pr, t0, tvals, tend, grads, rtol=1e-13, atol=1e-15):
    """Per-instance times: instance b starts at t0[b], is observed at tvals[b] (non-decreasing, repeats allowed) and its
    backward pass ends at tend[b] (t0[b] <= tend[b] <= tvals[b, 0]).

    Returns y_out [B, n_t, n]; sens [B, n_t, p, n], the forward sensitivities from t0 with S(t0) =
    initial_sensitivities(prob); grad_params [B, p] and grad_y_tend [B, n], dL/dp and dL/dy(tend) of
    L = sum_k g_k . y(t_k) for the system restarted at y(tend) with S = 0, S0 = I (what the backward pass that stops
    at tend returns as grad_out and -lamda_out); d_tvals [B, n_t] = f(t_k, y(t_k)) . g_k."""
    from sunode_amd.solver import initial_sensitivities
    n, p = prob.n_states, prob.n_params
    B, n_t = tvals.shape
    sens0 = initial_sensitivities(prob)
    rhs = augmented_rhs(prob)
    f = plain_rhs(prob)
    out = dict(y_out=np.zeros((B, n_t, n)), sens=np.zeros((B, n_t, p, n)), grad_params=np.zeros((B, p)),
               grad_y_tend=np.zeros((B, n)), d_tvals=np.zeros((B, n_t)))

    def run(ta, times, z0, psb, prb):
        """z at each of `times` (>= ta) of the augmented system started at (ta, z0)."""
        te = np.unique(times)
        if te[-1] == ta:                    # (nothing to integrate: every time is the start)
            return {ta: z0}
        sol = solve_ivp(rhs, (ta, te[-1]), z0, method="DOP853", t_eval=te, args=(psb, prb), rtol=rtol, atol=atol)
        assert sol.success, sol.message
        return dict(zip(te.tolist(), sol.y.T))

    for b in range(B):
        prb = pr if pr.ndim == 1 else pr[b]
        tv, g = tvals[b], grads[b]
        assert t0[b] <= tend[b] <= tv[0] and (np.diff(tv) >= 0).all()
        z0 = np.concatenate([y0[b], sens0.ravel(), np.eye(n).ravel()])
        zs = run(t0[b], np.append(tv, tend[b]), z0, ps[b], prb)
        z = np.array([zs[t] for t in tv.tolist()])
        out["y_out"][b] = z[:, :n]
        out["sens"][b] = z[:, n:n + n * p].reshape(n_t, p, n)
        if tend[b] != t0[b] or sens0.any():     # the gradient's system: S = 0, S0 = I at tend
            zr = run(tend[b], tv, np.concatenate([zs[tend[b]][:n], np.zeros(n * p), np.eye(n).ravel()]), ps[b], prb)
            z = np.array([zr[t] for t in tv.tolist()])
        S = z[:, n:n + n * p].reshape(n_t, p, n)
        S0 = z[:, n + n * p:].reshape(n_t, n, n)        # [k, j(y(tend) index), i(state)]
        out["grad_params"][b] = np.einsum("ki,kpi->p", g, S)
        out["grad_y_tend"][b] = np.einsum("ki,kji->j", g, S0)
        out["d_tvals"][b] = [f(t, out["y_out"][b, k], ps[b], prb) @ g[k] for k, t in enumerate(tv)]
        # d_tvals against a central difference of the truth solution: y(t_k +- h) of the plain ODE from (t0, y0)
        h = 1e-4
        ta, y0b = t0[b], y0[b]
        fwd_t = np.unique(np.concatenate([tv + h, tv - h]))
        lo, hi = fwd_t[fwd_t < ta], fwd_t[fwd_t >= ta]
        ys = {}
        for part, end in ((hi, hi[-1]), (lo[::-1], lo[0] if len(lo) else None)):
            if not len(part):
                continue
            sol = solve_ivp(lambda t, yv: f(t, yv, ps[b], prb), (ta, end), y0b, method="DOP853", t_eval=part,
                            rtol=rtol, atol=atol)
            assert sol.success, sol.message
            ys.update(zip(part.tolist(), sol.y.T))
        fd = np.array([(ys[(t + h)] - ys[(t - h)]) @ g[k] / ((t + h) - (t - h)) for k, t in enumerate(tv)])
        err = np.max(np.abs(fd - out["d_tvals"][b])) / np.abs(out["d_tvals"][b]).max()
        assert err < 1e-6, (b, err)
        print("  times instance %d: t0 %.6g, tend - t0 %.3g, span %.3g, d_tvals vs central difference %.1e"
              % (b, t0[b], tend[b] - t0[b], tv[-1] - t0[b], err), flush=True)
    return out


def _times_rows(B, n_t, t0, span, rng):
    """Grids t0 + span * sorted uniforms, with the edge rows of ``times_truth`` (its docstring names them)."""
    tv = t0[:, None] + span[:, None] * np.sort(rng.uniform(0.02, 1.0, (B, n_t)), axis=1)
    tend = t0.copy()
    for b in range(B):
        if b % 4 == 0:
            tv[b, 0] = t0[b]                            # first output time at t0
        elif b % 4 == 1:
            tv[b, :2] = t0[b]                           # t0 repeated at the head of the row
        elif b % 4 == 2:
            tend[b] = t0[b] + 0.5 * (tv[b, 0] - t0[b])  # backward pass stops before the forward start
        if b % 3 == 0:
            tv[b, n_t // 2 + 1] = tv[b, n_t // 2]       # a repeated output time inside the row
    return tv, tend


def times_truth():
    """truth_times_<name>.npz: per-instance start times, output grids and backward end times on the two models whose
    right-hand side reads t -- ``forcing`` (B-spline input on [0, 10], expit(k (t - t_mid))) and ``misc`` (sin t).

    Inputs t0 [B], tvals [B, n_t], tend [B], grads [B, n_t, n], y0, ps, pr (the models' own draws); truth y_out, sens,
    grad_params, grad_y_tend, d_tvals (``truth_times_batch``).  Keys ``one_*``: the same for a few rows with n_t = 1.

    Rows (B = 28, n_t = 8):
      * every b % 4 == 0: tvals[b, 0] == t0[b];  b % 4 == 1: tvals[b, 0] == tvals[b, 1] == t0[b];
        b % 4 == 2: t0[b] < tend[b] < tvals[b, 0] (tend halfway);  otherwise tend[b] == t0[b];
      * every b % 3 == 0: tvals[b, 5] == tvals[b, 4] (a repeated output time inside the row);
      * forcing: t0 spread over [-3, 7] (windows straddle the spline's support edge 0 and its knots); spans 0.02 on
        rows 0-3, 20 on rows 4-7, log-uniform in between on the rest (a factor 10^3 inside one wavefront); the
        cotangents of the rows shorter than 1 are scaled by 1 / span;
      * misc: t0 ~ 1e3 on rows 0-7 and ~ 1e5 on rows 8-15 with spans ~ 10 (UROUND |t| is no longer negligible in the
        initial step and the too-close test), t0 in [-5, 5] on the rest; spans 0.01 on rows 16-19.
    n_t = 1 rows (``one_*``, B = 6): tvals[b, 0] == t0[b] on row 0 (no forward step: its backward pass is CV_NO_FWD,
    the truth gradient there is not a solver's), tend halfway on rows 1 and 4."""
    for name, batch, B, n_t in (("forcing", forcing_batch, 28, 8), ("misc", misc_batch, 28, 8)):
        prob = make(name)
        n = prob.n_states
        rng = np.random.default_rng(7 if name == "forcing" else 11)
        d = batch(B)
        if name == "forcing":
            t0 = rng.uniform(-3.0, 7.0, B)
            span = 10.0 ** rng.uniform(np.log10(0.02), np.log10(20.0), B)
            span[:4], span[4:8] = 0.02, 20.0
        else:
            t0 = np.concatenate([1e3 + rng.uniform(-5.0, 5.0, 8), 1e5 + rng.uniform(-5.0, 5.0, 8),
                                 rng.uniform(-5.0, 5.0, B - 16)])
            span = rng.uniform(8.0, 12.0, B)
            span[16:20] = 0.01
        tvals, tend = _times_rows(B, n_t, t0, span, rng)
        # cotangents scaled by 1 / span on the short rows: their dL/dp stays O(1), as on the long rows, instead of
        # O(span) -- the absolute quadrature tolerance (1e-8) would otherwise be the error's floor there
        grads = _cotangents(B, n_t, n) * np.maximum(1.0, 1.0 / (tvals[:, -1] - t0))[:, None, None]
        res = truth_times_batch(prob, d["y0"], d["ps"], d["pr"], t0, tvals, tend, grads)
        # n_t = 1
        B1 = 6
        t01 = t0[:B1] + 0.25
        tv1 = t01[:, None] + rng.uniform(0.5, 3.0, (B1, 1))
        tv1[0, 0] = t01[0]
        tend1 = t01.copy()
        tend1[[1, 4]] = 0.5 * (t01[[1, 4]] + tv1[[1, 4], 0])
        g1 = _cotangents(B1, 1, n)
        res1 = truth_times_batch(prob, d["y0"][:B1], d["ps"][:B1], d["pr"], t01, tv1, tend1, g1)
        np.savez(os.path.join(GOLD, "truth_times_%s.npz" % name), y0=d["y0"], ps=d["ps"], pr=d["pr"], t0=t0,
                 tvals=tvals, tend=tend, grads=grads, **res,
                 one_t0=t01, one_tvals=tv1, one_tend=tend1, one_grads=g1, **{"one_" + k: v for k, v in res1.items()})


def main():
    os.makedirs(GOLD, exist_ok=True)
    if "--times" in sys.argv:
        times_truth()
        return
    if "--sweep" in sys.argv:
        sweep_truth()
        return
    for flag, models in FAMILY_FLAGS.items():
        if flag in sys.argv:
            for name in models:
                family_truth(name)
            return
    if "--nonsmooth" in sys.argv:
        nonsmooth_truth()
        return
    # ---------------- DVODE statistics ----------------
    def lv_f(t, y, a, b, c, d):
        return [a * y[0] - b * y[0] * y[1], d * y[0] * y[1] - c * y[1]]

    def lv_j(t, y, a, b, c, d):
        return [[a - b * y[1], -b * y[0]], [d * y[1], d * y[0] - c]]

    def rob_f(t, y, k1, k2, k3):
        return [-k1 * y[0] + k2 * y[1] * y[2], k1 * y[0] - k2 * y[1] * y[2] - k3 * y[1] ** 2, k3 * y[1] ** 2]

    def rob_j(t, y, k1, k2, k3):
        return [[-k1, k2 * y[2], k2 * y[1]], [k1, -k2 * y[2] - 2 * k3 * y[1], -k2 * y[1]], [0.0, 2 * k3 * y[1], 0.0]]

    stats = {}
    tv = np.linspace(0, 10)
    for tol in (1e-8, 1e-10):
        stats["lv_readme_%g" % tol] = dict(rtol=tol, atol=tol, tvals=tv.tolist(), y0=[1.0, 0.1],
                                           params=[0.1, 0.2, 0.3, 0.4],
                                           **dvode_run(lv_f, lv_j, [1.0, 0.1], tv, tol, tol, (0.1, 0.2, 0.3, 0.4)))
    lvb = lv_batch(8)
    for b in range(8):
        stats["lv_batch_%d" % b] = dict(rtol=1e-8, atol=1e-8, tvals=lvb["tvals"].tolist(), y0=lvb["y0"][b].tolist(),
                                        params=lvb["params"][b].tolist(),
                                        **dvode_run(lv_f, lv_j, lvb["y0"][b], lvb["tvals"], 1e-8, 1e-8, tuple(lvb["params"][b])))
    rb = robertson_batch(4)
    tv_long = np.array([0.0] + [0.4 * 10.0 ** k for k in range(12)])
    stats["robertson_4e10"] = dict(rtol=1e-8, atol=1e-10, tvals=tv_long.tolist(), y0=[1.0, 0.0, 0.0],
                                   params=[0.04, 1e4, 3e7],
                                   **dvode_run(rob_f, rob_j, [1.0, 0.0, 0.0], tv_long, 1e-8, 1e-10, (0.04, 1e4, 3e7)))
    stats["robertson_4e4"] = dict(rtol=1e-8, atol=1e-10, tvals=rb["tvals"].tolist(), y0=[1.0, 0.0, 0.0],
                                  params=[0.04, 1e4, 3e7],
                                  **dvode_run(rob_f, rob_j, [1.0, 0.0, 0.0], rb["tvals"], 1e-8, 1e-10, (0.04, 1e4, 3e7)))
    # step-by-step DVODE trace (ITASK=2) of the stiff transient: times and orders of the first steps
    import warnings
    r = ode(rob_f, rob_j).set_integrator("vode", method="bdf", with_jacobian=True, rtol=1e-8, atol=1e-10,
                                         nsteps=100000)
    r.set_initial_value([1.0, 0.0, 0.0], 0.0).set_f_params(0.04, 1e4, 3e7).set_jac_params(0.04, 1e4, 3e7)
    trace_t, trace_q = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        while r.t < 40.0:
            r.integrate(40.0, step=True)
            trace_t.append(float(r.t))
            trace_q.append(int(r._integrator.iwork[13]))
    iw = r._integrator.iwork
    stats["robertson_trace_T40"] = dict(t=trace_t, q=trace_q, nst=int(iw[10]), nfe=int(iw[11]), nje=int(iw[12]),
                                        nlu=int(iw[18]), nni=int(iw[19]), ncfn=int(iw[20]), netf=int(iw[21]))
    with open(os.path.join(GOLD, "dvode_stats.json"), "w") as fh:
        json.dump(stats, fh)
    print("dvode:", {k: (v["nst"], v["nfe"], v["nje"], v["nlu"], v["nni"], v["ncfn"], v["netf"])
                     for k, v in stats.items()})

    # ---------------- truth: LV config-2 batch (16 instances) ----------------
    prob = make("lv")
    B = 16
    d = lv_batch(B)
    ps = d["params"][:, prob.params_subset.subset_index]
    pr = d["params"][:, prob.params_subset.remainder_index]
    g = np.ones((len(d["tvals"]), 2))
    y_out, gp, gy0 = truth_batch(prob, d["y0"], ps, pr, d["t0"], d["tvals"], g, "DOP853")
    np.savez(os.path.join(GOLD, "truth_lv.npz"), y0=d["y0"], ps=ps, pr=pr, t0=d["t0"], tvals=d["tvals"],
             grads=g, y_out=y_out, grad_params=gp, grad_y0=gy0)

    # README instance with non-trivial cotangents
    rng_g = np.cos(np.arange(100.0)).reshape(50, 2)
    y_out, gp, gy0 = truth_batch(prob, np.array([[1.0, 0.1]]), np.array([[0.1, 0.2]]), np.array([[0.3, 0.4]]),
                                 0.0, np.linspace(0, 10), rng_g, "DOP853")
    np.savez(os.path.join(GOLD, "truth_lv_readme.npz"), y0=np.array([[1.0, 0.1]]), ps=np.array([[0.1, 0.2]]),
             pr=np.array([[0.3, 0.4]]), t0=0.0, tvals=np.linspace(0, 10), grads=rng_g, y_out=y_out,
             grad_params=gp, grad_y0=gy0)

    # ---------------- truth: Robertson config-3 (4 instances, Radau) ----------------
    prob = make("robertson")
    d = robertson_batch(4)
    g = cotangent(len(d["tvals"]), 3)
    y_out, gp, gy0 = truth_batch(prob, d["y0"], d["params"], np.zeros((4, 0)), d["t0"], d["tvals"], g, "Radau",
                                 rtol=1e-12, atol=1e-16)
    np.savez(os.path.join(GOLD, "truth_robertson.npz"), y0=d["y0"], ps=d["params"], pr=np.zeros((4, 0)),
             t0=d["t0"], tvals=d["tvals"], grads=g, y_out=y_out, grad_params=gp, grad_y0=gy0)

    # ---------------- truth: SEIR config-4 (2 instances) ----------------
    prob = make("seir")
    d = seir_batch(2)
    g = cotangent(len(d["tvals"]), 16)
    y_out, gp, gy0 = truth_batch(prob, d["y0"], d["ps"], d["pr"], d["t0"], d["tvals"], g, "DOP853")
    np.savez(os.path.join(GOLD, "truth_seir.npz"), y0=d["y0"], ps=d["ps"], pr=d["pr"], t0=d["t0"],
             tvals=d["tvals"], grads=g, y_out=y_out, grad_params=gp, grad_y0=gy0)
    for models in FAMILY_FLAGS.values():
        for name in models:
            family_truth(name)
    nonsmooth_truth()
    sweep_truth()
    print("done")


if __name__ == "__main__":
    main()
