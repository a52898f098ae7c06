"""Non-smooth right-hand sides: Abs, Max / Min, Piecewise, floor, Mod, sign and Heaviside from the generator to the oracle.

Models (tools/problems.py): ``nonsmooth_fn`` -- the catalogue of the forms, one or two per output; ``kinked`` -- a
continuous right-hand side with three kinks the solution crosses; ``threshold_sir4 / 8 / 16`` -- a grouped model whose
lanes sit on different branches (a lane family at 4 and 8 groups, SA_SUM terms at 16).

What is pinned here, without a device:
  (a) the generated C, compiled into the oracle, against ``sympy.evalf(40)`` of the ORIGINAL expressions at random points
      and at points ON every switching surface (dyadic coordinates, so that a tie is a tie in exact arithmetic too);
  (b) the two generator bugs of the issue: sign / Heaviside of a state (DiracDelta in the Jacobian) and the number
      symbols E, EulerGamma, Catalan, GoldenRatio, TribonacciConstant;
  (c) the oracle's forward + adjoint at rtol = atol = 1e-8 against DOP853 truth across the kinks;
  (d) the oracle's forward sensitivities of ``kinked`` against the truth's.
The device's side of it -- bit for bit against the oracle -- is tests/test_gpu_nonsmooth.py, which uses the points of (a).
"""
import functools
import os
import re
import warnings

import numpy as np
import pytest
import sympy as sym

from tests.helpers import make_oracle, make_problem

DIGITS = 40
NAMES = ("nonsmooth_fn", "kinked", "threshold_sir4", "threshold_sir8", "threshold_sir16")
KEYS = ("rhs", "jac", "adj", "quad", "adjjac")

#: (a): 4 x the worst error |generated - sympy| / max(1, |sympy|) over the points of ``points(name)``, every callback.
#: Measured (test_generated_callbacks_equal_sympy prints them): nonsmooth_fn 4.3e-16, kinked 8.7e-17, threshold_sir4
#: 6.5e-16, threshold_sir8 4.3e-15 (a quadrature entry of 0.7 left by cancelling terms of order 10), threshold_sir16 7.1e-16.
CALLBACK_BARS = {"nonsmooth_fn": 1.7e-15, "kinked": 3.5e-16, "threshold_sir4": 2.6e-15, "threshold_sir8": 1.7e-14,
                 "threshold_sir16": 2.8e-15}

#: (c), (d): 3 x the oracle's measured error at rtol = atol = 1e-8 (see the tests' docstrings), in the measures of
#: tools/make_golden_truth.py ``truth_errors``
TRUTH_BARS = {"kinked": dict(y=6.9e-7, grad_params=9.1e-7, grad_y0=8.6e-7, sens=4.3e-6),
              "threshold_sir8": dict(y=1.3e-6, grad_params=3.1e-6, grad_y0=4.6e-6)}


# ----------------------------------------------------------------------------------------------------------------------
# points
def _dyadic(rng, shape, lo=2, hi=24):
    """Multiples of 1/8 in [lo / 8, hi / 8]: sums, differences and products of a few of them are exact in fp64."""
    return rng.randint(lo, hi + 1, shape) / 8.0


def _nonsmooth_fn_points():
    rng = np.random.RandomState(5)
    N = 24
    y = rng.uniform(0.3, 2.5, (N, 5))
    a = rng.uniform(0.3, 2.2, (N, 5))
    a[::2, 1] *= -1.0
    t = rng.uniform(0.0, 4.0, N)
    rows = [(t[i], y[i], a[i]) for i in range(N)]

    def tie(edit, tval=None):
        yy, aa = _dyadic(rng, 5), _dyadic(rng, 5)
        edit(yy, aa)
        rows.append((rng.randint(0, 32) / 8.0 + 0.0625 if tval is None else tval, yy, aa))

    def set_(arr, i, v):
        arr[i] = v

    # x0 == a0 with a1 of either sign: a1 (x0 - a0) is +0 or -0 (the tie of Max(., 0), Abs(0), Heaviside(0), Piecewise edge)
    tie(lambda y_, a_: (set_(y_, 0, a_[0]), set_(a_, 1, -abs(a_[1]))))
    tie(lambda y_, a_: (set_(y_, 0, a_[0]), set_(a_, 1, abs(a_[1]))))
    tie(lambda y_, a_: (set_(y_, 0, a_[0]), set_(a_, 1, -0.75), set_(y_, 1, 0.5)))
    tie(lambda y_, a_: set_(y_, 1, a_[1] * y_[2]))                                  # Max(x1, a1 x2)
    tie(lambda y_, a_: set_(y_, 3, y_[0]))                                          # Min(x0, x3, a3): x0 == x3
    tie(lambda y_, a_: set_(a_, 3, y_[3]))                                          # ... x3 == a3; Piecewise x3 < a3
    tie(lambda y_, a_: (set_(a_, 3, y_[0]), set_(y_, 3, y_[0])))                    # ... all three equal
    tie(lambda y_, a_: set_(a_, 2, y_[0]))                                          # Max(x0, a2)
    tie(lambda y_, a_: set_(y_, 1, a_[0] * y_[3]))                                  # Max(x1, a0 x3)
    tie(lambda y_, a_: (set_(y_, 0, 2.0), set_(a_, 2, 1.0)))                        # Min(., ., 2): first argument == 2
    tie(lambda y_, a_: (set_(y_, 0, 2.5), set_(a_, 2, 1.0), set_(y_, 1, 2.0), set_(a_, 0, 0.5), set_(y_, 3, 1.0)))
    tie(lambda y_, a_: set_(a_, 2, y_[2]))                                          # Max(0, x2 - a2)**2
    tie(lambda y_, a_: set_(y_, 3, y_[2]))                                          # Max(x2, x3, a4)
    tie(lambda y_, a_: set_(a_, 4, max(y_[2], y_[3])))
    tie(lambda y_, a_: set_(a_, 0, y_[2]))                                          # Ne(x2, a0): the equal branch
    tie(lambda y_, a_: set_(a_, 0, y_[1]))                                          # sign(x1 - a0) == 0
    tie(lambda y_, a_: (set_(a_, 1, 0.5), set_(a_, 0, 0.5), set_(y_, 0, 2.5), set_(y_, 1, 1.0)))   # x1 == Max(a1 (x0 - a0), 0)
    for tval in (1.0, 2.0, 1.5, 0.0, 3.0, 4.0, -0.0, 0.5):                          # Heaviside / And / sign / floor / Mod
        tie(lambda y_, a_: None, tval)
    tt = np.array([r[0] for r in rows])
    yy = np.array([r[1] for r in rows])
    aa = np.array([r[2] for r in rows])
    lam = np.concatenate([rng.randn(N, 5), _dyadic(rng, (len(rows) - N, 5), -16, 16)])
    return tt, yy, lam, aa, np.zeros((len(rows), 0)), N


def _kinked_points():
    rng = np.random.RandomState(6)
    N = 12
    y = rng.uniform(0.05, 1.2, (N, 3))
    ps = rng.uniform(0.2, 1.5, (N, 4))
    rows = [(y[i], ps[i]) for i in range(N)]
    for which in ((0,), (1,), (2,), (0, 1, 2)):
        for _ in range(2):
            yy, pp = _dyadic(rng, 3, 1, 12), _dyadic(rng, 4, 1, 12)
            if 0 in which:
                yy[0] = pp[1]               # x == c
            if 1 in which:
                yy[1] = pp[0]               # y == th
            if 2 in which:
                yy[2] = 0.25                # z == 1/4
            rows.append((yy, pp))
    yy = np.array([r[0] for r in rows])
    pp = np.array([r[1] for r in rows])
    lam = np.concatenate([rng.randn(N, 3), _dyadic(rng, (len(rows) - N, 3), -16, 16)])
    return rng.uniform(0, 5, len(rows)), yy, lam, pp, np.zeros((len(rows), 0)), N


def _threshold_sir_points(M):
    from tools.problems import threshold_sir_batch
    rng = np.random.RandomState(7 + M)
    N = 3 if M == 16 else 6
    d = threshold_sir_batch(N, M)
    y = d["y0"] * np.exp(0.3 * rng.randn(N, 2 * M))
    rows = [(y[i], d["ps"][i]) for i in range(N)]
    for k in range(2 if M == 16 else 4):
        yy = np.concatenate([_dyadic(rng, M, 40, 100), _dyadic(rng, M, 2, 24)])
        pp = np.concatenate([_dyadic(rng, M, 1, 4) / 8.0, [0.25, 1.0 + 0.125 * k]])
        yy[M + (3 * k) % M] = pp[-1]        # I[j] == th
        yy[M + (3 * k + 1) % M] = 1.0       # I[i] == 1: the edge of the recovery Piecewise
        if k % 2:
            yy[M + (3 * k + 2) % M] = pp[-1]
        rows.append((yy, pp))
    yy = np.array([r[0] for r in rows])
    pp = np.array([r[1] for r in rows])
    lam = np.concatenate([rng.randn(N, 2 * M), _dyadic(rng, (len(rows) - N, 2 * M), -16, 16)])
    C = np.round(d["pr"] * 64.0) / 64.0     # (dyadic: the tie points stay exact through the contact matrix)
    return rng.uniform(0, 5, len(rows)), yy, lam, pp, np.tile(C, (len(rows), 1)), N


@functools.lru_cache(maxsize=None)
def points(name):
    """-> (t [N], y [N, n], lam [N, n], ps [N, p], pr [N, r], number of leading random points): random points, then
    points on every switching surface of the model."""
    if name == "nonsmooth_fn":
        return _nonsmooth_fn_points()
    if name == "kinked":
        return _kinked_points()
    return _threshold_sir_points(int(name[len("threshold_sir"):]))


# ----------------------------------------------------------------------------------------------------------------------
# (a) generated C against sympy
def _exact(x):
    return sym.Float(float(x), DIGITS)          # (a double is 53 bits: exact at 40 digits)


def sympy_callbacks(prob, t, y, lam, ps, pr):
    """The five callbacks from the ORIGINAL symbolic arrays of ``prob`` at one point, 40 digits, DiracDelta -> 0."""
    sub = {prob._sym_time: _exact(t)}
    sub.update({s: _exact(v) for s, v in zip(prob._sym_statevec, y)})
    sub.update({s: _exact(v) for s, v in zip(prob._sym_lamda, lam)})
    sub.update({s: _exact(v) for s, v in zip(prob._sym_deriv_paramsvec, ps)})
    sub.update({s: _exact(v) for s, v in zip(prob._sym_fixed_paramsvec, pr)})

    def value(e):
        e = sym.sympify(e).replace(sym.DiracDelta, lambda *args: sym.Integer(0))
        v = sym.N(e.xreplace(sub), DIGITS)
        assert v.is_number and not v.free_symbols, e
        return v
    n = prob.n_states
    jac = np.array([[value(prob._sym_dydt_jac[i, j]) for j in range(n)] for i in range(n)], dtype=object)
    return dict(rhs=np.array([value(e) for e in prob._sym_dydt], dtype=object), jac=jac,
                adj=np.array([value(e) for e in prob._sym_dlamdadt], dtype=object),
                quad=np.array([value(e) for e in prob._sym_quad_rhs], dtype=object), adjjac=-jac.T)


def exact_mask(name, key, shape, on_surface):
    """Outputs made only of exactly rounded operations on the inputs (compare, select, fabs, sa_min / sa_max, floor, fmod
    and ONE + - x /): they must equal the correctly rounded reference.
      nonsmooth_fn: row 1 of the Jacobian, a1 x Heaviside x Heaviside (products with 0, 1/2, 1), and its image in the
        adjoint Jacobian, at every point; output 1 itself, Min(Max(a1 (x0 - a0), 0), x1), at the dyadic surface points
        (there the difference and the product are both exact; at a random point they are two roundings);
      kinked: the whole Jacobian and adjoint Jacobian (+-parameter, +-1, sign / 5, a select of 1 and 2)."""
    mask = np.zeros(shape, dtype=bool)
    if name == "nonsmooth_fn":
        if key == "jac":
            mask[1, :] = True
        elif key == "adjjac":
            mask[:, 1] = True
        elif key == "rhs" and on_surface:
            mask[1] = True
    elif name == "kinked" and key in ("jac", "adjjac"):
        mask[...] = True
    return mask


@pytest.mark.parametrize("name", NAMES)
def test_generated_callbacks_equal_sympy(name):
    """orc.eval against evalf(40) of ``_sym_dydt``, ``_sym_dlamdadt``, ``_sym_quad_rhs``, the Jacobian and the adjoint
    Jacobian.  Exactly rounded outputs (``exact_mask``): equal to the rounded reference.  Everything else: within 4 x the
    worst error measured on these points, relative to max(1, |value|) -- measured nonsmooth_fn 4.3e-16, kinked 8.7e-17,
    threshold_sir4 6.5e-16, threshold_sir8 4.3e-15, threshold_sir16 7.1e-16; bars ``CALLBACK_BARS``."""
    prob = make_problem(name)
    orc = make_oracle(name)
    t, y, lam, ps, pr, n_random = points(name)
    worst = 0.0
    n_exact = 0
    for i in range(len(t)):
        got = orc.eval(t[i], y[i], lam[i], ps[i], pr[i])
        ref = sympy_callbacks(prob, t[i], y[i], lam[i], ps[i], pr[i])
        assert np.asarray(got["codes"]).tolist() == [0] * 5
        for key in KEYS:
            g, r = np.asarray(got[key]), ref[key]
            exact = exact_mask(name, key, g.shape, i >= n_random)
            for idx in np.ndindex(g.shape):
                err = float(abs(_exact(g[idx]) - r[idx]) / max(1, abs(r[idx])))
                if exact[idx]:
                    n_exact += 1
                    assert g[idx] == float(r[idx]), (name, i, key, idx, g[idx], r[idx])
                worst = max(worst, err)
                assert err <= CALLBACK_BARS[name], (name, i, key, idx, err, g[idx], r[idx])
    print("%s: worst error against sympy %.2e (bar %.1e), %d exactly rounded outputs" % (name, worst, CALLBACK_BARS[name],
                                                                                           n_exact))
    assert n_exact > 0 or name.startswith("threshold_sir")


def test_points_sit_on_every_switching_surface():
    """(what (a) and the device comparison are made on) nonsmooth_fn: every Max / Min has a point with two equal
    arguments, every Piecewise / Heaviside / sign a point on its edge, t is 1, 2, 3/2 and an integer; x0 == a0 comes
    with a1 of either sign (a1 (x0 - a0) is -0 or +0: the tie of Max(., 0)) and output 1 is +0 there, as the rule of
    sa_max says -- with the inherited fmax the oracle's answer was -0 where the product was."""
    t, y, lam, a, _, n_random = points("nonsmooth_fn")
    ts, ys, as_ = t[n_random:], y[n_random:], a[n_random:]
    ties = {
        "x0 == a0, a1 < 0": (ys[:, 0] == as_[:, 0]) & (as_[:, 1] < 0), "x0 == a0, a1 > 0": (ys[:, 0] == as_[:, 0]) & (as_[:, 1] > 0),
        "x1 == a1 x2": ys[:, 1] == as_[:, 1] * ys[:, 2], "x0 == x3": ys[:, 0] == ys[:, 3], "x3 == a3": ys[:, 3] == as_[:, 3],
        "x0 == a2": ys[:, 0] == as_[:, 2], "x1 == a0 x3": ys[:, 1] == as_[:, 0] * ys[:, 3],
        "Max(x0, a2) == 2": np.maximum(ys[:, 0], as_[:, 2]) == 2.0, "x2 == a2": ys[:, 2] == as_[:, 2], "x2 == x3": ys[:, 2] == ys[:, 3],
        "a4 == Max(x2, x3)": as_[:, 4] == np.maximum(ys[:, 2], ys[:, 3]), "x2 == a0": ys[:, 2] == as_[:, 0],
        "x1 == a0": ys[:, 1] == as_[:, 0], "x1 == Max(a1 (x0 - a0), 0)": ys[:, 1] == np.maximum(as_[:, 1] * (ys[:, 0] - as_[:, 0]), 0),
    }
    for label, hit in ties.items():
        assert hit.any(), label
    for tval in (1.0, 2.0, 1.5, 0.0, 3.0):
        assert (ts == tval).any(), tval
    assert (y > 0).all()
    orc = make_oracle("nonsmooth_fn")
    zeros = [orc.eval(t[i], y[i], lam[i], a[i], np.zeros(0))["rhs"][1] for i in range(len(t)) if y[i, 0] == a[i, 0]]
    assert len(zeros) >= 3 and all(z == 0.0 and not np.signbit(z) for z in zeros), zeros
    _, yk, _, pk, _, nk = points("kinked")
    assert (yk[nk:, 0] == pk[nk:, 1]).any() and (yk[nk:, 1] == pk[nk:, 0]).any() and (yk[nk:, 2] == 0.25).any()
    for M in (4, 8, 16):
        _, ym, _, pm, _, nm = points("threshold_sir%d" % M)
        assert (ym[nm:, M:] == pm[nm:, -1:]).any(axis=1).all() and (ym[nm:, M:] == 1.0).any(axis=1).all()
        above = (ym[:nm, M:] > pm[:nm, -1:]).sum(axis=1)
        assert ((above > 0) & (above < M)).all()            # random points: lanes of one instance on both branches of Max
        on = (ym[nm:, M:] == pm[nm:, -1:]).sum(axis=1)
        assert ((on > 0) & (on < M)).all()                  # surface points: some groups ON the threshold, others not


@pytest.mark.parametrize("M,marker", [(4, "SA_FAM_BEGIN(4)"), (8, "SA_FAM_BEGIN(8)"), (16, "SA_SUM(")])
def test_threshold_sir_structure(M, marker):
    """The grouped threshold model is a lane family at 4 and 8 groups (one group per lane: the select inside
    SA_FAM_BEGIN) and re-rolled sums at 16 (one term per lane: the select inside an SA_SUM term)."""
    src = make_problem("threshold_sir%d" % M).native_source()
    body = src[src.index("SA_TEMPLATE SA_FN int sa_rhs"):]
    assert marker in body
    assert ("SA_FAM_BEGIN" in body) == (M != 16) and ("SA_SUM(" in body) == (M == 16)
    if M == 16:         # the state-dependent select sits inside a rolled term
        assert any("sa_max(" in line for line in body.splitlines() if "SA_SUM(" in line)
    else:               # ... inside the family region
        assert "sa_max(" in body[body.index(marker):body.index("SA_FAM_END")]


# ----------------------------------------------------------------------------------------------------------------------
# (b) the two generator bugs
def _header_is_clean(src):
    body = src[src.index("SA_TEMPLATE SA_FN int sa_rhs"):]
    assert not re.search(r"\bM_[A-Z0-9_]+\b", body), re.findall(r"\bM_[A-Z0-9_]+\b", body)
    for line in body.splitlines():         # (a declaration after an '=' of the same statement: "v_ = const double E = ...")
        assert line.startswith("SA_TEMPLATE") or not re.search(r"=[^;]*\bconst double\b", line), line
    assert "DiracDelta" not in body


def _small_problem(rhs, params=None):
    from sunode_amd import SympyProblem
    params = params or {"a": (), "b": ()}
    return SympyProblem(params, {"x": (), "z": ()}, rhs, [(k,) for k in params])


def _compiled(prob, tag):
    from oracle.harness import Oracle
    return Oracle(prob, tag=tag)


@pytest.mark.parametrize("fn", ["sign", "Heaviside"])
def test_sign_and_heaviside_of_a_state_generate_and_warn(fn):
    """d sign(u) = 2 DiracDelta(u), d Heaviside(u) = DiracDelta(u): printed as 0.0, the derivative almost everywhere --
    the Jacobian sympy derives for the same switch written as a Piecewise --, and announced by a UserWarning that names
    the function and the missing jump term."""
    f = getattr(sym, fn)
    prob = _small_problem(lambda t, y, p: {"x": -p.a * y.x + p.b * f(y.z - p.a), "z": y.x - y.z * f(y.x - 1)})
    with pytest.warns(UserWarning, match=r"%s\(.*jump term" % fn) as rec:
        src = prob.native_source()
    assert all(w.category is UserWarning for w in rec)
    _header_is_clean(src)
    orc = _compiled(prob, "delta_" + fn)
    pw = {"sign": lambda u: sym.Piecewise((-1, u < 0), (0, sym.Eq(u, 0)), (1, True)),
          "Heaviside": lambda u: sym.Piecewise((0, u < 0), (sym.Rational(1, 2), sym.Eq(u, 0)), (1, True))}[fn]
    twin = _small_problem(lambda t, y, p: {"x": -p.a * y.x + p.b * pw(y.z - p.a), "z": y.x - y.z * pw(y.x - 1)})
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        orc_twin = _compiled(twin, "delta_%s_piecewise" % fn)
    for y in ([0.5, 2.0], [1.0, 0.75], [1.5, 0.25], [1.0, 0.5]):
        a, b = orc.eval(0.3, y, [0.25, -1.5], [0.75, 1.25], np.zeros(0)), orc_twin.eval(0.3, y, [0.25, -1.5], [0.75, 1.25], np.zeros(0))
        for key in KEYS:
            np.testing.assert_array_equal(a[key], b[key], err_msg="%s %s" % (key, y))
        assert a["codes"].tolist() == [0] * 5


def test_a_switch_in_time_has_no_delta_and_no_warning():
    """Heaviside(t - 1) with a literal switching time: no derivative of it is taken, nothing is left out."""
    prob = _small_problem(lambda t, y, p: {"x": -p.a * y.x + p.b * sym.Heaviside(t - 1) + sym.sign(t - 2), "z": y.x - y.z})
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        src = prob.native_source()
    _header_is_clean(src)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _header_is_clean(make_problem("switched").native_source())


def test_a_parameter_dependent_switching_time_warns():
    """Heaviside(t - a) with a DIFFERENTIATED a: df/da is a delta -- the gradient with respect to a lacks its jump."""
    prob = _small_problem(lambda t, y, p: {"x": -p.b * y.x + sym.Heaviside(t - p.a), "z": y.x - y.z})
    with pytest.warns(UserWarning, match="jump term"):
        prob.native_source()


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64).tolist()


def test_max_min_tie_and_nan_rule():
    """``Max / Min`` are printed as ``sa_max / sa_min`` (codegen.MINMAX_C), never as fmax / fmin -- the device's and the
    host's fmax answered the +-0 tie differently (tests/test_gpu_nonsmooth.py, the -0 product under Max(., 0)).  The
    rule, on the compiled header: -0 < +0 in either argument order, a NaN operand is ignored, NaN only if both are;
    three arguments nest."""
    from sunode_amd.symode import codegen
    prob = _small_problem(lambda t, y, p: {"x": sym.Max(p.a, p.b), "z": sym.Min(p.a, p.b)})
    src = prob.native_source()
    assert codegen.MINMAX_C in src and "sa_max(" in src and "sa_min(" in src
    assert not re.search(r"\bf(max|min)\(", src)
    assert codegen.MINMAX_C not in make_problem("lv").native_source()          # (only where it is called)
    orc = _compiled(prob, "minmax_rule")
    nan = float("nan")
    for a, b, want_max, want_min in ((0.0, -0.0, 0.0, -0.0), (-0.0, 0.0, 0.0, -0.0), (-0.0, -0.0, -0.0, -0.0),
                                     (0.0, 0.0, 0.0, 0.0), (nan, 1.5, 1.5, 1.5), (1.5, nan, 1.5, 1.5), (nan, -0.0, -0.0, -0.0),
                                     (2.0, 2.0, 2.0, 2.0), (-3.0, 2.0, 2.0, -3.0), (float("inf"), -float("inf"), float("inf"), -float("inf"))):
        got = orc.eval(0.0, [1.0, 1.0], [0.0, 0.0], [a, b], np.zeros(0))
        assert _bits(got["rhs"]) == _bits([want_max, want_min]), (a, b, got["rhs"])
    got = orc.eval(0.0, [1.0, 1.0], [0.0, 0.0], [nan, nan], np.zeros(0))
    assert np.isnan(got["rhs"]).all() and got["codes"][0] == 1
    three = _small_problem(lambda t, y, p: {"x": sym.Max(p.a, p.b, y.z - 1), "z": sym.Min(p.a, p.b, y.z - 1, 2)})
    got = _compiled(three, "minmax_three").eval(0.0, [1.0, 1.0], [0.0, 0.0], [-0.0, -0.0], np.zeros(0))
    assert _bits(got["rhs"]) == _bits([0.0, -0.0])                              # z - 1 = +0 among two -0


NUMBER_SYMBOLS = ("E", "EulerGamma", "Catalan", "GoldenRatio", "TribonacciConstant", "pi")


def test_number_symbols_are_literals():
    """Every number symbol as a coefficient, as a power and inside a sum: the header compiles (no declaration spliced
    into a statement, no M_* macro) and the value is the correctly rounded constant."""
    consts = [getattr(sym, n) for n in NUMBER_SYMBOLS]

    def rhs(t, y, p):
        return {"x": sum(c * y.x ** k for k, c in enumerate(consts)) + p.a,
                "z": y.z * sym.E ** 2 + sym.pi / 2 + 2 / sym.sqrt(sym.pi) * p.b + sym.sqrt(2) + sym.log(2) * y.z + 1 / sym.EulerGamma}
    prob = _small_problem(rhs)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        src = prob.native_source()
    _header_is_clean(src)
    for c in consts:
        assert repr(float(c.evalf(30))) in src, c
    orc = _compiled(prob, "number_symbols")
    got = orc.eval(0.0, [1.0, 0.0], [0.0, 0.0], [0.0, 0.0], np.zeros(0))
    # x = 1, z = 0, a = b = 0: output 0 is the sum of the constants, output 1 is pi / 2 + sqrt(2) + 1 / EulerGamma
    ref0 = sum(consts).evalf(30)
    ref1 = (sym.pi / 2 + sym.sqrt(2) + 1 / sym.EulerGamma).evalf(30)
    assert abs(got["rhs"][0] - float(ref0)) <= 4 * np.spacing(float(ref0))
    assert abs(got["rhs"][1] - float(ref1)) <= 4 * np.spacing(float(ref1))
    # one constant alone: exactly its rounded value (x^k = 1 exactly)
    for k, c in enumerate(consts):
        single = _small_problem(lambda t, y, p, c=c: {"x": c * y.x, "z": p.a + p.b + c})
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            one = _compiled(single, "number_symbol_%s" % NUMBER_SYMBOLS[k]).eval(0.0, [1.0, 0.0], [0.0, 0.0], [0.0, 0.0], np.zeros(0))
        assert one["rhs"][0] == float(c.evalf(30)) and one["rhs"][1] == float(c.evalf(30)), c
        _header_is_clean(single.native_source())


@pytest.mark.parametrize("name", NAMES)
def test_no_macro_and_no_spliced_declaration_in_the_model_headers(name):
    _header_is_clean(make_problem(name).native_source())


# ----------------------------------------------------------------------------------------------------------------------
# (c), (d) truth
def _truth(golden_dir, name):
    return np.load(os.path.join(golden_dir, "truth_%s.npz" % name))


@functools.lru_cache(maxsize=None)
def oracle_run(name, golden_dir):
    """Forward + adjoint of the truth fixture's draws in the oracle at rtol = atol = 1e-8 (computed once)."""
    d = _truth(golden_dir, name)
    orc = make_oracle(name)
    cfg = orc.config(rtol=1e-8, atol=1e-8, rtolB=1e-8, atolB=1e-8, rtolQB=1e-8, atolQB=1e-8)
    tv = d["tvals"]
    y, st, stats = orc.solve_forward(cfg, d["y0"], d["ps"], d["pr"], float(d["t0"]), tv, nthreads=4)
    g, lam, stb, statsb = orc.solve_backward(cfg, tv[-1], float(d["t0"]), tv, d["grads"], nthreads=4)
    return dict(y_out=y, grad_params=g, grad_y0=-lam, status=st, status_b=stb, stats=stats, stats_b=statsb)


def test_kinked_fixture_crosses_its_surfaces():
    """A condition on the fixture (tools/problems.py kinked_batch), read from the truth trajectories: at least three
    quarters of the draws cross ALL three surfaces x = c, y = th, z = 1/4 between two output times, transversally (the
    surface function's derivative along the solution has the crossing's sign at both bracketing outputs and is at
    least 0.02 there); the rest stay on one side of at least one surface; and the crossing times of every surface are
    spread over at least 0.3 between draws -- dozens of steps of a solver at rtol 1e-8 (0.01 ... 0.05 there)."""
    from tools.problems import KINKED_Q
    golden_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    d = _truth(golden_dir, "kinked")
    orc = make_oracle("kinked")
    y, ps, tv = d["y_out"], d["ps"], d["tvals"]
    B = len(y)
    level = np.stack([ps[:, 1], ps[:, 0], np.full(B, KINKED_Q)], axis=1)            # of x, y, z
    s = y - level[:, None, :]                                                       # [B, n_t, surface]
    crossing = np.full((B, 3), np.nan)
    for b in range(B):
        f = np.array([orc.eval(tv[k], y[b, k], np.zeros(3), ps[b], np.zeros(0))["rhs"] for k in range(len(tv))])
        for j in range(3):
            ks = np.nonzero(np.sign(s[b, 1:, j]) != np.sign(s[b, :-1, j]))[0]
            if not len(ks):
                continue
            k = ks[0]
            direction = np.sign(s[b, k + 1, j] - s[b, k, j])
            if direction * f[k, j] >= 0.02 and direction * f[k + 1, j] >= 0.02:
                crossing[b, j] = tv[k] + (tv[k + 1] - tv[k]) * s[b, k, j] / (s[b, k, j] - s[b, k + 1, j])
    all_three = ~np.isnan(crossing).any(axis=1)
    assert all_three.mean() >= 0.75, crossing
    rest = ~all_three
    assert rest.any()
    one_sided = (np.abs(np.sign(s).sum(axis=1)) == s.shape[1]).any(axis=1)          # same strict side at every output
    assert one_sided[rest].all(), crossing
    spread = np.nanmax(crossing, axis=0) - np.nanmin(crossing, axis=0)
    assert (spread >= 0.3).all(), spread


@pytest.mark.parametrize("name", ["kinked", "threshold_sir8"])
def test_truth_fixture_is_converged(name, golden_dir):
    """The fixture's own error: its two DOP853 runs (rtol 1e-13 and 1e-11) agree 100 times tighter than the bars."""
    d = _truth(golden_dir, name)
    assert len(d["y0"]) == 8
    for key, bar in TRUTH_BARS[name].items():
        assert float(d["agree_" + key]) * 100 <= bar, (key, float(d["agree_" + key]))


@pytest.mark.parametrize("name", ["kinked", "threshold_sir8"])
def test_oracle_forward_adjoint_matches_truth_across_kinks(name, golden_dir):
    """Oracle at rtol = atol = 1e-8 against DOP853 truth, 8 draws, every status 0.  Measured (max over the batch, measures
    of ``truth_errors``): kinked states 2.3e-7, dL/dp 3.0e-7, dL/dy0 2.9e-7; threshold_sir8 states 4.1e-7,
    dL/dp 1.0e-6, dL/dy0 1.5e-6.  Bars ``TRUTH_BARS``: 3 x these, per model and quantity."""
    from tools.make_golden_truth import truth_errors
    d = _truth(golden_dir, name)
    run = oracle_run(name, golden_dir)
    assert (run["status"] == 0).all() and (run["status_b"] == 0).all()
    err = truth_errors(run, d)
    print(name, "oracle against truth:", err)
    for key in ("y", "grad_params", "grad_y0"):
        assert err[key] <= TRUTH_BARS[name][key], (key, err[key])


def test_oracle_forward_sensitivities_match_truth_across_kinks(golden_dir):
    """CVODES-style forward sensitivities (simultaneous corrector) of ``kinked`` against the truth's dy/dp at every
    output time, in the measure of ``truth_errors``.  Measured 1.43e-6 (states of that run: 1.0e-7); bar 3 x that: ``TRUTH_BARS``."""
    from tools.make_golden_truth import truth_errors
    d = _truth(golden_dir, "kinked")
    orc = make_oracle("kinked")
    sens0 = np.zeros((4, 3))
    y, sens, st, _ = orc.solve_sens(orc.config(rtol=1e-8, atol=1e-8), d["y0"], d["ps"], d["pr"], sens0, float(d["t0"]),
                                    d["tvals"], mode="simultaneous", nthreads=4)
    assert (st == 0).all()
    err = truth_errors(dict(y_out=y, grad_params=d["grad_params"], grad_y0=d["grad_y0"], sens=sens), d)
    print("kinked forward sensitivities against truth:", err)
    assert err["sens"] <= TRUTH_BARS["kinked"]["sens"], err
    assert err["y"] <= TRUTH_BARS["kinked"]["y"], err
