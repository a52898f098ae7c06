"""Inverse trigonometric / inverse hyperbolic functions and erf / erfc in generated right-hand sides -- the CPU half.

* ``csrc/sa_math_inv.h`` (the second block of the math library, embedded after ``csrc/sa_math.h`` into the headers
  that call one of its functions): accuracy against mpmath at 200 bits (ceiling 4 ulp, the worst bound sa_math.h
  states for its own functions), special values (C99 Annex F), both sides of every interval boundary;
* the code generator: the nine functions are printed as ``sa_*`` calls, nothing of them is left to libm, models
  without them keep their header; ``SympyProblem`` warns about the functions that still are libm-only;
* the callbacks of ``mathfn_c`` / ``mathfn_d`` against hand-written closed forms of the values and first derivatives
  (mpmath, 40 digits: nothing of sympy's differentiation or of the printers on that side);
* the oracle on ``probit_gate`` against DOP853 truth (tools/make_golden_truth.py --inverse-erf).

The GPU half (device == oracle bit for bit, device vs truth) is tests/test_gpu_inverse_erf.py.
"""
import ctypes
import os
import warnings

import numpy as np
import pytest

from tests.family_checks import compile_math_blocks
from tests.helpers import make_oracle, make_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = ["asin", "acos", "atan", "asinh", "acosh", "atanh", "erf", "erfc"]
NINE = ONE + ["atan2"]
ULP_CEILING = 4.0
TINY = 2.2250738585072014e-308          # smallest normal double


@pytest.fixture(scope="module")
def mathlib():
    """sa_math.h + sa_math_inv.h compiled for the host exactly like the oracle compiles a generated header."""
    L = compile_math_blocks(("core", "inv"), [
        "void w_%s(int n, const double *x, double *o) { for (int i = 0; i < n; i++) o[i] = sa_%s(x[i]); }" % (f, f)
        for f in ONE] + ["void w_atan2(int n, const double *y, const double *x, double *o) "
                         "{ for (int i = 0; i < n; i++) o[i] = sa_atan2(y[i], x[i]); }"])

    def call(name, x, y=None):
        x = np.ascontiguousarray(x, float)
        o = np.empty_like(x)
        vp = ctypes.c_void_p
        if y is None:
            getattr(L, "w_" + name)(len(x), vp(x.ctypes.data), vp(o.ctypes.data))
        else:
            y = np.ascontiguousarray(y, float)
            getattr(L, "w_" + name)(len(x), vp(x.ctypes.data), vp(y.ctypes.data), vp(o.ctypes.data))
        return o
    return call


def _mp():
    import mpmath as mp
    mp.mp.prec = 200
    return mp


def _reference(name):
    mp = _mp()
    return {"asin": mp.asin, "acos": mp.acos, "atan": mp.atan, "asinh": mp.asinh, "acosh": mp.acosh, "atanh": mp.atanh,
            "erf": mp.erf, "erfc": mp.erfc, "atan2": mp.atan2}[name]


def _ulps(got, ref):
    """Worst error in ulps of the true value; a subnormal true value: absolute error in subnormal steps."""
    mp = _mp()
    worst = 0.0
    for g, r in zip(got, ref):
        rf = float(r)
        assert np.isfinite(g), (g, rf)
        if rf == 0.0:
            assert g == 0.0, (g, r)
            continue
        worst = max(worst, float(abs(mp.mpf(float(g)) - r) / np.spacing(abs(rf))))
    return worst


def _points():
    rng = np.random.RandomState(0)
    N = 1500

    def sgn():
        return rng.choice([-1.0, 1.0], N)
    near_one = (1.0 - rng.uniform(0, 1e-8, N)) * sgn()
    pts = {
        "asin": np.concatenate([rng.uniform(-1, 1, N), near_one]),
        "acos": np.concatenate([rng.uniform(-1, 1, N), near_one]),
        "atan": 10.0 ** rng.uniform(-20, 20, N) * sgn(),
        "asinh": 10.0 ** rng.uniform(-20, 300, N) * sgn(),
        "acosh": 1.0 + 10.0 ** rng.uniform(-16, 300, N),
        "atanh": np.concatenate([(1.0 - 10.0 ** rng.uniform(-16, 0, N)) * sgn(), 10.0 ** rng.uniform(-20, 0, N) * sgn()]),
        "erf": 10.0 ** rng.uniform(-20, 1, N) * sgn(),
        "erfc": rng.uniform(-6, 26.5, N),
    }
    two = (10.0 ** rng.uniform(-10, 10, N) * sgn(), 10.0 ** rng.uniform(-10, 10, N) * sgn())      # (y, x): four quadrants
    return pts, two


def test_accuracy_against_mpmath(mathlib):
    """<= 4 ulp for every function over the ranges of the issue (1 500 random points per range); subnormal erfc
    results within one subnormal step."""
    mp = _mp()
    pts, (y2, x2) = _points()
    worst = {}
    for name, x in pts.items():
        f = _reference(name)
        worst[name] = _ulps(mathlib(name, x), [f(mp.mpf(float(v))) for v in x])
    worst["atan2"] = _ulps(mathlib("atan2", y2, x2), [mp.atan2(mp.mpf(float(a)), mp.mpf(float(b))) for a, b in zip(y2, x2)])
    print("worst ulp:", {k: round(v, 2) for k, v in worst.items()})
    for name, w in worst.items():
        assert w <= ULP_CEILING, (name, w)
    # the erfc tail: relative accuracy down to the smallest normal result, one subnormal step below it
    x = np.concatenate([np.linspace(25.0, 26.5, 301), np.linspace(26.5, 27.3, 161)])
    got = mathlib("erfc", x)
    for v, g in zip(x, got):
        r = mp.erfc(mp.mpf(float(v)))
        if r >= TINY:
            assert abs(mp.mpf(float(g)) - r) <= ULP_CEILING * np.spacing(float(r)), (v, g)
        else:
            assert abs(mp.mpf(float(g)) - r) <= mp.mpf(5e-324), (v, g)


def test_special_values(mathlib):
    inf, nan, pi = np.inf, np.nan, np.pi

    def same(got, want):
        """equal values AND equal signs of zero; NaN where NaN is wanted"""
        got, want = np.asarray(got), np.asarray(want, float)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(np.signbit(got)[~np.isnan(want)], np.signbit(want)[~np.isnan(want)])
    same(mathlib("asin", [0.0, -0.0, 1.0, -1.0, 1.0000000000000002, -2.0, inf, nan]), [0.0, -0.0, pi / 2, -pi / 2, nan, nan, nan, nan])
    same(mathlib("acos", [1.0, -1.0, 0.0, 1.0000000000000002, -2.0, -inf, nan]), [0.0, pi, pi / 2, nan, nan, nan, nan])
    same(mathlib("atan", [0.0, -0.0, inf, -inf, nan, 1e300, -1e300]), [0.0, -0.0, pi / 2, -pi / 2, nan, pi / 2, -pi / 2])
    same(mathlib("asinh", [0.0, -0.0, inf, -inf, nan]), [0.0, -0.0, inf, -inf, nan])
    same(mathlib("acosh", [1.0, 0.9999999999999999, 0.0, -3.0, inf, -inf, nan]), [0.0, nan, nan, nan, inf, nan, nan])
    same(mathlib("atanh", [0.0, -0.0, 1.0, -1.0, 1.0000000000000002, -7.0, inf, nan]), [0.0, -0.0, inf, -inf, nan, nan, nan, nan])
    same(mathlib("erf", [0.0, -0.0, inf, -inf, nan, 30.0, -30.0]), [0.0, -0.0, 1.0, -1.0, nan, 1.0, -1.0])
    same(mathlib("erfc", [0.0, -0.0, inf, -inf, nan, 28.0, -28.0]), [1.0, 1.0, 0.0, 2.0, nan, 0.0, 2.0])
    # atan2(y, x): the zero / infinity / sign table of C99 F.9.1.4
    table = [
        (0.0, 1.0, 0.0), (-0.0, 1.0, -0.0), (0.0, 0.0, 0.0), (-0.0, 0.0, -0.0),
        (0.0, -1.0, pi), (-0.0, -1.0, -pi), (0.0, -0.0, pi), (-0.0, -0.0, -pi),
        (1.0, 0.0, pi / 2), (1.0, -0.0, pi / 2), (-1.0, 0.0, -pi / 2), (-1.0, -0.0, -pi / 2),
        (inf, 3.0, pi / 2), (-inf, -3.0, -pi / 2), (inf, 0.0, pi / 2),
        (inf, inf, pi / 4), (-inf, inf, -pi / 4), (inf, -inf, 3 * pi / 4), (-inf, -inf, -3 * pi / 4),
        (2.0, inf, 0.0), (-2.0, inf, -0.0), (2.0, -inf, pi), (-2.0, -inf, -pi), (0.0, inf, 0.0), (-0.0, -inf, -pi),
        (nan, 1.0, nan), (1.0, nan, nan), (nan, nan, nan), (nan, inf, nan), (0.0, nan, nan),
    ]
    y, x, want = (np.array(c) for c in zip(*table))
    same(mathlib("atan2", y, x), want)


def test_both_sides_of_every_interval_boundary(mathlib):
    """The boundaries come from the header's own definitions (codegen.math_boundaries("inv")): 41 consecutive doubles
    around each one, and around its mirror image for the odd / two-sided functions, stay within the ulp ceiling."""
    from sunode_amd.symode import codegen
    mp = _mp()
    bounds = codegen.math_boundaries("inv")
    assert set(bounds) == set(NINE) and all(len(b) >= 1 for b in bounds.values())
    assert len(bounds["atan"]) == 4 and len(bounds["erf"]) == 5 and len(bounds["erfc"]) >= 6
    for name, bs in bounds.items():
        f = _reference(name)
        for b in bs:
            x = [b]
            for _ in range(20):
                x = [np.nextafter(x[0], -np.inf)] + x + [np.nextafter(x[-1], np.inf)]
            x = np.array(x)
            sides = [x] if name in ("acosh", "erfc") else [x, -x]
            for xs in sides:
                if name == "atan2":                       # the quotient |y / x| crosses the boundary: (y, x) = (b, +-1), (+-1, 1/b)
                    for yy, xx in ((xs, np.ones_like(xs)), (xs, -np.ones_like(xs))):
                        got = mathlib("atan2", yy, xx)
                        w = _ulps(got, [mp.atan2(mp.mpf(float(a)), mp.mpf(float(c))) for a, c in zip(yy, xx)])
                        assert w <= ULP_CEILING, (name, b, w)
                    continue
                w = _ulps(mathlib(name, xs), [f(mp.mpf(float(v))) for v in xs])
                assert w <= ULP_CEILING, (name, b, w)


NEW_MODELS = ("mathfn_c", "mathfn_d", "probit_gate")


def test_generated_source_calls_the_deterministic_functions_only():
    from sunode_amd.symode import codegen
    for name in NEW_MODELS:
        src = make_problem(name).native_source()
        assert "SA_HAVE_MATH" in src and "SA_HAVE_MATH_INV" in src
        assert src.index("#endif /* SA_MATH_H */") < src.index("#ifndef SA_MATH_INV_H")
        assert codegen.libm_calls(src) == [], name            # (the parent commit returned the nine names here)
    both = make_problem("mathfn_c").native_source() + make_problem("mathfn_d").native_source()
    body = make_problem("probit_gate").native_source().split("#endif /* SA_MATH_INV_H */")[1]
    for fn in NINE:
        assert "sa_%s(" % fn in both, fn
        assert "sa_%s(" % fn in body, fn
    for name in ("misc", "lv", "forcing"):
        assert "SA_HAVE_MATH_INV" not in make_problem(name).native_source()
    assert not set(NINE) & set(codegen.LIBM_ONLY)


def _hypot_model():
    import sympy as sym
    from sympy.codegen.cfunctions import hypot
    from sunode_amd import SympyProblem

    def rhs(t, y, p):
        return {"x": -p.k * hypot(y.x, y.z), "z": sym.atan(y.x) - y.z}
    return SympyProblem({"k": ()}, {"x": (), "z": ()}, rhs, [("k",)])


def test_libm_only_functions_warn_once_and_the_new_functions_do_not():
    from sunode_amd import SympyProblem
    from sunode_amd.symode import codegen
    from tools.problem_cache import spec_of
    with pytest.warns(UserWarning, match="hypot") as rec:
        prob = _hypot_model()
        src = prob.native_source()
        prob.native_source()
    assert codegen.libm_calls(src) == ["hypot"]
    mine = [w for w in rec if "hypot" in str(w.message)]
    assert len(mine) == 1 and "bit" in str(mine[0].message)
    s = spec_of("probit_gate")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        SympyProblem(s["params"], s["states"], s["rhs"], s["derivative_params"]).native_source()


def _closed_forms(name, x, a, lam):
    """Values f_i(x_i, a_i) of ``mathfn_c`` / ``mathfn_d`` and their partial derivatives, written by hand (mpmath)."""
    import mpmath as mp
    x = [mp.mpf(float(v)) for v in x]
    a = [mp.mpf(float(v)) for v in a]
    sp = mp.sqrt(mp.pi)
    if name == "mathfn_c":
        f = [mp.asin(a[0] * x[0]), mp.acos(x[1] / a[1]), mp.atan(a[2] * x[2]), mp.atan2(x[3], a[3]),
             mp.atan2(a[4], x[4] - 2) + mp.asin(x[4] / a[4])]
        fx = [a[0] / mp.sqrt(1 - (a[0] * x[0]) ** 2), -1 / (a[1] * mp.sqrt(1 - (x[1] / a[1]) ** 2)),
              a[2] / (1 + (a[2] * x[2]) ** 2), a[3] / (x[3] ** 2 + a[3] ** 2),
              -a[4] / ((x[4] - 2) ** 2 + a[4] ** 2) + 1 / (a[4] * mp.sqrt(1 - (x[4] / a[4]) ** 2))]
        fa = [x[0] / mp.sqrt(1 - (a[0] * x[0]) ** 2), x[1] / (a[1] ** 2 * mp.sqrt(1 - (x[1] / a[1]) ** 2)),
              x[2] / (1 + (a[2] * x[2]) ** 2), -x[3] / (x[3] ** 2 + a[3] ** 2),
              (x[4] - 2) / ((x[4] - 2) ** 2 + a[4] ** 2) - x[4] / (a[4] ** 2 * mp.sqrt(1 - (x[4] / a[4]) ** 2))]
    else:
        f = [mp.asinh(a[0] * x[0]), mp.acosh(1 + a[1] * x[1]), mp.atanh(x[2] / a[2]), mp.erf(a[3] * x[3]),
             mp.erfc(x[4] / a[4]) + mp.erf(x[4])]
        u1 = 1 + a[1] * x[1]
        fx = [a[0] / mp.sqrt(1 + (a[0] * x[0]) ** 2), a[1] / mp.sqrt(u1 ** 2 - 1), (1 / a[2]) / (1 - (x[2] / a[2]) ** 2),
              2 * a[3] / sp * mp.exp(-(a[3] * x[3]) ** 2),
              -2 / (sp * a[4]) * mp.exp(-(x[4] / a[4]) ** 2) + 2 / sp * mp.exp(-x[4] ** 2)]
        fa = [x[0] / mp.sqrt(1 + (a[0] * x[0]) ** 2), x[1] / mp.sqrt(u1 ** 2 - 1),
              (-x[2] / a[2] ** 2) / (1 - (x[2] / a[2]) ** 2), 2 * x[3] / sp * mp.exp(-(a[3] * x[3]) ** 2),
              2 * x[4] / (sp * a[4] ** 2) * mp.exp(-(x[4] / a[4]) ** 2)]
    n = 5
    J = np.zeros((n, n))
    J[np.arange(n), np.arange(n)] = [float(v) for v in fx]          # f_i depends on x_i and a_i only
    fa = np.array([float(v) for v in fa])
    return dict(rhs=np.array([float(v) for v in f]), jac=J, adj=-lam @ J, quad=lam * fa, adjjac=-J.T)


@pytest.mark.parametrize("name", ["mathfn_c", "mathfn_d"])
def test_callbacks_against_hand_written_closed_forms(name):
    """64 points inside every function's domain: the oracle's five callbacks against closed forms of the values and
    first derivatives, rtol 1e-13 (the bar of tests/helpers.check_matrix_summary)."""
    import mpmath as mp
    mp.mp.dps = 40
    orc = make_oracle(name)
    rng = np.random.RandomState(3)
    for _ in range(64):
        x = rng.uniform(0.05, 0.9, 5)
        a = rng.uniform(1.02, 1.1, 5)         # a x < 1 and x / a < 1: inside the domains of asin / acos / atanh
        lam = rng.randn(5)
        got = orc.eval(0.0, x, lam, a, np.zeros(0))
        want = _closed_forms(name, x, a, lam)
        assert np.asarray(got["codes"]).tolist() == [0] * 5
        for key in ("rhs", "jac", "adj", "quad", "adjjac"):
            g = np.asarray(got[key], float)
            w = want[key]
            if key in ("jac", "adjjac"):
                g = g.reshape(5, 5, order="F")
            np.testing.assert_allclose(g, w, rtol=1e-13, atol=64 * 2.3e-16 * np.abs(w).max(), err_msg="%s %s" % (name, key))


def test_oracle_forward_adjoint_matches_truth_on_probit_gate(golden_dir):
    """The bars of tests/test_gpu_transcendental.py at rtol = atol = 1e-8: states <= 1e-5, gradients and -lamda <= 4e-6
    relative to the per-draw maximum, against DOP853 truth (16 draws)."""
    d = np.load(os.path.join(golden_dir, "truth_probit_gate.npz"))
    assert d["y0"].shape[0] == 16
    orc = make_oracle("probit_gate")
    cfg = orc.config(rtol=1e-8, atol=1e-8, rtolB=1e-8, atolB=1e-8, rtolQB=1e-8, atolQB=1e-8)
    tv = d["tvals"]
    y, st, _ = orc.solve_forward(cfg, d["y0"], d["ps"], d["pr"], float(d["t0"]), tv, nthreads=4)
    g, lam, stb, _ = orc.solve_backward(cfg, tv[-1], float(d["t0"]), tv, d["grads"], nthreads=4)
    assert (st == 0).all() and (stb == 0).all()
    assert np.max(np.abs(y - d["y_out"]) / np.abs(d["y_out"]).max(axis=(0, 1))) < 1e-5
    assert np.max(np.abs(g - d["grad_params"]) / np.abs(d["grad_params"]).max(axis=1, keepdims=True)) < 4e-6
    assert np.max(np.abs(-lam - d["grad_y0"]) / np.abs(d["grad_y0"]).max(axis=1, keepdims=True)) < 4e-6
