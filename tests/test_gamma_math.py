"""Gamma, loggamma, digamma and trigamma in generated right-hand sides -- the CPU half.

* ``csrc/sa_math_gamma.h`` (the third block of the math library, embedded after ``csrc/sa_math.h`` -- and
  ``csrc/sa_math_inv.h`` where present -- into the headers that call one of its functions): accuracy against mpmath at
  200 bits, special values, both sides of every piece boundary.  Ceiling: 4 ulp (``ULP_CEILING`` of
  tests/test_inverse_erf_math.py, the worst bound sa_math.h states), with two stated exceptions: lgamma / digamma at
  x < 0 go through a reflection formula that cancels, so their error is counted in units of
  spacing(max(|f(x)|, |f(1 - x)|)); tgamma's ceiling on a set of points is max(4 ulp, the worst error of
  scipy.special.gamma -- the function the reference's printer emits -- on the same points), computed here, no margin
  (subnormal results of tgamma, which scipy rounds to 0: the plain 4, in steps of 2^-1074); an underflowed tgamma is a
  zero with the sign of Gamma over a seeded sample down to -3e15;
* the code generator: gamma / loggamma / digamma / trigamma / polygamma(0 | 1, .) / factorial are printed as ``sa_*``
  calls, nothing of them is left to libm, no warning; models without them keep their header byte for byte (sha256 of
  ``native_source()`` recorded on the parent commit); polygamma(n >= 2, .) raises;
* the callbacks of ``mathfn_e`` against hand-written closed forms of the values and first derivatives (mpmath,
  40 digits: nothing of sympy's differentiation or of the printers on that side);
* the oracle on ``gamma_delay`` against DOP853 truth (tools/make_golden_truth.py --gamma).

The GPU half (device == oracle bit for bit, device vs truth) is tests/test_gpu_gamma.py.
"""
import ctypes
import hashlib
import json
import os
import warnings

import numpy as np
import pytest

from tests.family_checks import compile_math_blocks
from tests.helpers import make_oracle, make_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOUR = ["lgamma", "tgamma", "digamma", "trigamma"]
ULP_CEILING = 4.0
N_POINTS = 1500
PSI_ROOT = 1.4616321449683622            # the positive root of digamma


@pytest.fixture(scope="module")
def mathlib():
    """sa_math.h + sa_math_inv.h + sa_math_gamma.h compiled for the host exactly like the oracle compiles a generated
    header."""
    L = compile_math_blocks(("core", "inv", "gamma"), [
        "void w_%s(int n, const double *x, double *o) { for (int i = 0; i < n; i++) o[i] = sa_%s(x[i]); }" % (f, f)
        for f in FOUR])

    def call(name, x):
        x = np.ascontiguousarray(x, float)
        o = np.empty_like(x)
        getattr(L, "w_" + name)(len(x), ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(o.ctypes.data))
        return o
    return call


def _mp():
    import mpmath as mp
    mp.mp.prec = 200
    return mp


def _reference(name):
    mp = _mp()
    return {"lgamma": lambda v: mp.loggamma(v) if v > 0 else mp.log(abs(mp.gamma(v))),       # log|Gamma|
            "tgamma": mp.gamma, "digamma": lambda v: mp.psi(0, v), "trigamma": lambda v: mp.psi(1, v)}[name]


def _worst(name, x, got, reflected=False):
    """Worst error of ``got`` against mpmath, in ulps of the true value -- ``reflected``: in units of
    spacing(max(|f(x)|, |f(1 - x)|)), the size of the terms the reflection formula subtracts."""
    mp = _mp()
    f = _reference(name)
    worst = 0.0
    for xv, g in zip(x, got):
        r = f(mp.mpf(float(xv)))
        assert np.isfinite(g), (name, xv, g)
        size = abs(float(r))
        if reflected:
            size = max(size, abs(float(f(1 - mp.mpf(float(xv))))))
        if size == 0.0:
            assert g == 0.0, (name, xv, g)
            continue
        worst = max(worst, float(abs(mp.mpf(float(g)) - r) / np.spacing(size)))
    return worst


def _negative_zeros(name):
    """Zeros of lgamma / digamma in (-12, 0) that lie at least 1e-3 away from the poles: bracketed on a grid with
    scipy.special, located with mpmath.findroot."""
    from scipy import special
    mp = _mp()
    f = _reference(name)
    coarse = special.gammaln if name == "lgamma" else special.digamma
    zeros = []
    for k in range(-12, 0):
        grid = np.linspace(k + 1e-3, k + 1 - 1e-3, 4001)
        v = coarse(grid)
        for i in np.nonzero(np.sign(v[:-1]) * np.sign(v[1:]) < 0)[0]:
            zeros.append(float(mp.findroot(f, (mp.mpf(float(grid[i])), mp.mpf(float(grid[i + 1]))), solver="anderson")))
    return np.array(zeros)


def _off_integers(x):
    return x[np.abs(x - np.round(x)) >= 1e-3]


def _ranges():
    """{function: {range: (points, reflected)}}: the ranges of the issue, 1 500 seeded points each.  Negative ranges
    exclude points within 1e-3 of an integer and, for lgamma / digamma, within 1e-3 of a zero of the function."""
    rng = np.random.RandomState(0)
    N = N_POINTS

    def around(c):
        return c + rng.choice([-1.0, 1.0], N) * 10.0 ** rng.uniform(-12, -1, N)

    def negative(name, lo=-12.0):
        x = _off_integers(rng.uniform(lo, 0, N))
        if name in ("lgamma", "digamma"):
            z = _negative_zeros(name)
            assert len(z) >= (12 if name == "digamma" else 8), (name, z)      # (lgamma's other zeros hug the poles)
            x = x[np.min(np.abs(x[:, None] - z[None, :]), axis=1) >= 1e-3]
        assert len(x) > 0.9 * N
        return x
    return {
        "lgamma": {"10^U(-300,300)": (10.0 ** rng.uniform(-300, 300, N), False), "U(0,30)": (rng.uniform(0, 30, N), False),
                   "1+-10^U(-12,-1)": (around(1.0), False), "2+-10^U(-12,-1)": (around(2.0), False),
                   "U(-12,0)": (negative("lgamma"), True)},
        "tgamma": {"U(0,171.6)": (rng.uniform(0, 171.6, N), False), "10^U(-300,0)": (10.0 ** rng.uniform(-300, 0, N), False),
                   "U(-170,0)": (negative("tgamma", -170.0), False),
                   # subnormal results (what the 2^-128 rescaling of the far path is for): np.spacing is 2^-1074 there
                   # (own seed: the other ranges keep their points; scipy.special.gamma returns 0 there, so this range
                   # has the plain ceiling: 4 steps)
                   "U(-184,-170.6) plain": (_off_integers(np.random.RandomState(1).uniform(-184.0, -170.6, N)), False)},
        "digamma": {"10^U(-300,300)": (10.0 ** rng.uniform(-300, 300, N), False), "U(0,30)": (rng.uniform(0, 30, N), False),
                    "x0+-10^U(-12,-1)": (around(PSI_ROOT), False), "U(-12,0)": (negative("digamma"), True)},
        "trigamma": {"10^U(-150,300)": (10.0 ** rng.uniform(-150, 300, N), False), "U(0,30)": (rng.uniform(0, 30, N), False),
                     "U(-12,0)": (negative("trigamma"), False)},
    }


def _ceiling(name, x, label=""):
    """4 ulp; tgamma: max(4 ulp, the worst error of scipy.special.gamma on the same points)."""
    if name != "tgamma" or label.endswith("plain"):
        return ULP_CEILING
    from scipy import special
    return max(ULP_CEILING, _worst("tgamma", x, special.gamma(x)))


def test_accuracy_against_mpmath(mathlib):
    """Every function over the ranges of the issue: within the ceiling of its range; the measured worst cases are
    printed (the header comment carries them)."""
    worst, ceil = {}, {}
    for name, ranges in _ranges().items():
        for label, (x, reflected) in ranges.items():
            worst[name, label] = _worst(name, x, mathlib(name, x), reflected)
            ceil[name, label] = _ceiling(name, x, label)
    for (name, label), w in worst.items():
        print("worst error %-9s %-18s %.2f (ceiling %.2f)" % (name, label, w, ceil[name, label]))
    for key, w in worst.items():
        assert w <= ceil[key], (key, w, ceil[key])


def test_special_values(mathlib):
    inf, nan = np.inf, np.nan

    def same(got, want):
        """equal values AND equal signs of zero; NaN where NaN is wanted"""
        got, want = np.asarray(got), np.asarray(want, float)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(np.signbit(got)[~np.isnan(want)], np.signbit(want)[~np.isnan(want)])
    poles = [0.0, -0.0, -1.0, -2.0, -3.0, -170.0, -1e15, -1e300]
    same(mathlib("lgamma", poles + [inf, -inf, nan, 1.0, 2.0, 1e306, 3e305]), [inf] * 8 + [inf, inf, nan, 0.0, 0.0, inf, inf])
    same(mathlib("tgamma", poles + [inf, -inf, nan]), [inf, -inf] + [nan] * 6 + [inf, nan, nan])
    same(mathlib("digamma", poles + [inf, -inf, nan]), [nan] * 8 + [inf, nan, nan])
    same(mathlib("trigamma", poles + [inf, -inf, nan]), [inf] * 8 + [0.0, nan, nan])
    # Gamma at the integers is the factorial (exact in a double up to 22!): within the ceiling
    import math
    n = np.arange(1.0, 24.0)
    want = np.array([float(math.factorial(int(v) - 1)) for v in n])
    assert (np.abs(mathlib("tgamma", n) - want) <= ULP_CEILING * np.spacing(want)).all()
    # overflow above 171.62..., the last finite value below it
    same(mathlib("tgamma", [171.7, 172.0, 1e10, 1e308]), [inf] * 4)
    assert np.isfinite(mathlib("tgamma", [171.6243769563027])[0]) and mathlib("tgamma", [171.6243769563027])[0] > 1.79e308
    # underflow to +-0 with the sign of Gamma on (-n - 1, -n): negative for an even n
    same(mathlib("tgamma", [-200.5, -201.5, -1000.25, -1001.25, -4.5e15 + 0.5]), [-0.0, 0.0, -0.0, 0.0, 0.0])
    # ... on a seeded sample of 4 000 negative non-integers from -185 down to -3e15: every result is a zero whose sign is
    # that of Gamma, negative where floor(-x) is even
    rng = np.random.RandomState(5)
    x = -(10.0 ** rng.uniform(np.log10(185.0), 15.5, 4000))
    x = x[x != np.round(x)]
    assert len(x) > 3900
    got = mathlib("tgamma", x)
    assert (got == 0.0).all()
    np.testing.assert_array_equal(np.signbit(got), np.floor(-x) % 2 == 0)
    # tiny arguments: Gamma(x) = 1/x, lgamma = -log|x|, psi = -1/x, psi' = 1/x^2
    same(mathlib("tgamma", [1e-300, -1e-300, 5e-324, -5e-324]), [1.0 / 1e-300, -1.0 / 1e-300, inf, -inf])
    same(mathlib("trigamma", [1e-200, -1e-200]), [inf, inf])
    got = mathlib("digamma", [1e-300, -1e-300])
    np.testing.assert_allclose(got, [-1e300, 1e300], rtol=1e-15)
    got = mathlib("lgamma", [1e-300, -1e-300])
    np.testing.assert_allclose(got, [690.7755278982137, 690.7755278982137], rtol=1e-15)


def test_both_sides_of_every_piece_boundary(mathlib):
    """The boundaries come from the header's own definitions (codegen.math_boundaries("gamma")): 41 consecutive doubles
    around each one -- and around its mirror image on the negative axis where that is not a pole (lgamma reflects to
    -x) -- stay within the ceilings of the accuracy test."""
    from sunode_amd.symode import codegen
    bounds = codegen.math_boundaries("gamma")
    assert set(bounds) == set(FOUR)
    assert len(bounds["lgamma"]) >= 5 and len(bounds["tgamma"]) == 6 and len(bounds["digamma"]) == 4 and len(bounds["trigamma"]) == 4
    for name, bs in bounds.items():
        for b in bs:
            x = [b]
            for _ in range(20):
                x = [np.nextafter(x[0], -np.inf)] + x + [np.nextafter(x[-1], np.inf)]
            x = np.array(x)
            w = _worst(name, x, mathlib(name, x))
            assert w <= _ceiling(name, x), (name, b, w)
            if name == "lgamma" and b != np.round(b):
                w = _worst(name, -x, mathlib(name, -x), reflected=True)
                assert w <= ULP_CEILING, (name, -b, w)


NEW_MODELS = ("mathfn_e", "gamma_delay")


def test_new_models_build_without_a_warning_and_call_the_deterministic_functions_only():
    from sunode_amd import SympyProblem
    from sunode_amd.symode import codegen
    from tools.problem_cache import spec_of
    for name in NEW_MODELS:
        s = spec_of(name)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            src = SympyProblem(s["params"], s["states"], s["rhs"], s["derivative_params"]).native_source()
        assert src == make_problem(name).native_source()
        assert codegen.libm_calls(src) == [], name
        assert "SA_HAVE_MATH_GAMMA" in src and "SA_HAVE_MATH_INV" not in src
        assert src.index("#endif /* SA_MATH_H */") < src.index("#ifndef SA_MATH_GAMMA_H")
        body = src.split("#endif /* SA_MATH_GAMMA_H */")[1]
        for fn in FOUR:
            assert "sa_%s(" % fn in body, (name, fn)
    assert not {"tgamma", "lgamma"} & set(codegen.LIBM_ONLY)


def test_the_block_comes_after_the_inverse_block_where_both_are_present():
    import sympy as sym
    from sunode_amd import SympyProblem

    def rhs(t, y, p):
        return {"x": sym.atan(y.x) - p.k * sym.loggamma(1 + y.x * y.x)}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        src = SympyProblem({"k": ()}, {"x": ()}, rhs, [("k",)]).native_source()
    assert src.index("#endif /* SA_MATH_H */") < src.index("#endif /* SA_MATH_INV_H */") < src.index("#ifndef SA_MATH_GAMMA_H")


def test_existing_headers_keep_their_text(golden_dir):
    with open(os.path.join(golden_dir, "native_source_sha256.json")) as fh:
        digests = json.load(fh)
    for name in ("lv", "misc", "forcing", "logistic_switch", "mathfn_a", "mathfn_c", "probit_gate"):
        src = make_problem(name).native_source()
        assert "SA_HAVE_MATH_GAMMA" not in src
        assert hashlib.sha256(src.encode()).hexdigest() == digests[name], name


def test_polygamma_beyond_trigamma_raises():
    import sympy as sym
    from sunode_amd import SympyProblem

    def rhs(t, y, p):
        return {"x": -p.k * sym.trigamma(y.x)}
    with pytest.raises(NotImplementedError, match=r"polygamma\(2"):
        SympyProblem({"k": ()}, {"x": ()}, rhs, [("k",)]).native_source()


def test_gamma_of_a_remainder_parameter_is_deterministic_and_silent():
    import sympy as sym
    from sunode_amd import SympyProblem
    from sunode_amd.symode import codegen

    def rhs(t, y, p):
        return {"x": -p.k * y.x * sym.gamma(p.fixed) + sym.loggamma(p.fixed)}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        src = SympyProblem({"k": (), "fixed": ()}, {"x": ()}, rhs, [("k",)]).native_source()
    body = src.split("#endif /* SA_MATH_GAMMA_H */")[1]
    assert "sa_tgamma(" in body and "sa_lgamma(" in body and codegen.libm_calls(src) == []


def test_host_helpers_evaluate_the_family():
    """``HOST_FUNCTIONS`` (sympy.lambdify of a model's expressions on the host) knows the six names."""
    import sympy as sym
    from scipy import special
    from sunode_amd.symode.problem import HOST_FUNCTIONS
    u = sym.Symbol("u")
    expr = [sym.gamma(u), sym.loggamma(u), sym.digamma(u), sym.trigamma(u), sym.polygamma(0, u), sym.polygamma(1, u),
            sym.factorial(u)]
    fn = sym.lambdify([u], expr, modules=[HOST_FUNCTIONS, "numpy"])
    for v in (0.3, 2.5, -1.5):
        want = [special.gamma(v), special.gammaln(v), special.digamma(v), special.polygamma(1, v), special.digamma(v),
                special.polygamma(1, v), special.gamma(v + 1)]
        np.testing.assert_allclose(np.asarray(fn(v), float), want, rtol=1e-14)


def _closed_forms(x, a, lam):
    """Values f_i(x_i, a_i) of ``mathfn_e`` and their partial derivatives, written by hand (mpmath)."""
    import mpmath as mp
    x = [mp.mpf(float(v)) for v in x]
    a = [mp.mpf(float(v)) for v in a]

    def lg(u):
        return mp.log(abs(mp.gamma(u)))

    def psi(u):
        return mp.psi(0, u)

    def psi1(u):
        return mp.psi(1, u)
    u = [a[0] * x[0], x[1] / a[1], a[2] * x[2], a[3] * x[3], 1 + a[4] * x[4]]
    v3 = x[3] / a[3]
    f = [lg(u[0]), mp.gamma(u[1]), psi(u[2]), lg(u[3]) + psi(v3), mp.gamma(u[4])]
    fx = [a[0] * psi(u[0]), mp.gamma(u[1]) * psi(u[1]) / a[1], a[2] * psi1(u[2]), a[3] * psi(u[3]) + psi1(v3) / a[3],
          a[4] * mp.gamma(u[4]) * psi(u[4])]
    fa = [x[0] * psi(u[0]), -x[1] / a[1] ** 2 * mp.gamma(u[1]) * psi(u[1]), x[2] * psi1(u[2]),
          x[3] * psi(u[3]) - x[3] / a[3] ** 2 * psi1(v3), x[4] * mp.gamma(u[4]) * psi(u[4])]
    n = 5
    J = np.zeros((n, n))
    J[np.arange(n), np.arange(n)] = [float(v) for v in fx]          # f_i depends on x_i and a_i only
    fa = np.array([float(v) for v in fa])
    return dict(rhs=np.array([float(v) for v in f]), jac=J, adj=-lam @ J, quad=lam * fa, adjjac=-J.T)


def test_callbacks_against_hand_written_closed_forms():
    """64 points: the oracle's five callbacks of ``mathfn_e`` against closed forms of the values and first derivatives,
    at the bar of ``mathfn_c`` / ``mathfn_d`` (rtol 1e-13, tests/helpers.check_matrix_summary).  x[3] takes both signs,
    so that the arguments a x and x / a of output 3 cross zero and the negative axis (kept 0.05 away from the poles)."""
    import mpmath as mp
    mp.mp.dps = 40
    orc = make_oracle("mathfn_e")
    rng = np.random.RandomState(3)
    done = negative = 0
    while done < 64:
        x = rng.uniform(0.05, 0.9, 5)
        a = rng.uniform(1.02, 1.1, 5)
        x[3] = rng.uniform(-2.4, 2.4)
        args = np.array([a[3] * x[3], x[3] / a[3]])
        if np.abs(args - np.round(args)).min() < 0.05:
            continue
        done += 1
        negative += x[3] < 0
        lam = rng.randn(5)
        got = orc.eval(0.0, x, lam, a, np.zeros(0))
        want = _closed_forms(x, a, lam)
        assert np.asarray(got["codes"]).tolist() == [0] * 5
        for key in ("rhs", "jac", "adj", "quad", "adjjac"):
            g = np.asarray(got[key], float)
            w = want[key]
            if key in ("jac", "adjjac"):
                g = g.reshape(5, 5, order="F")
            np.testing.assert_allclose(g, w, rtol=1e-13, atol=64 * 2.3e-16 * np.abs(w).max(), err_msg=key)
    assert 16 <= negative <= 48


def test_oracle_forward_adjoint_matches_truth_on_gamma_delay(golden_dir):
    """The bars of tests/test_gpu_transcendental.py at rtol = atol = 1e-8: states <= 1e-5, gradients and -lamda <= 4e-6
    relative to the per-draw maximum, against DOP853 truth (16 draws)."""
    d = np.load(os.path.join(golden_dir, "truth_gamma_delay.npz"))
    assert d["y0"].shape[0] == 16
    orc = make_oracle("gamma_delay")
    cfg = orc.config(rtol=1e-8, atol=1e-8, rtolB=1e-8, atolB=1e-8, rtolQB=1e-8, atolQB=1e-8)
    tv = d["tvals"]
    y, st, _ = orc.solve_forward(cfg, d["y0"], d["ps"], d["pr"], float(d["t0"]), tv, nthreads=4)
    g, lam, stb, _ = orc.solve_backward(cfg, tv[-1], float(d["t0"]), tv, d["grads"], nthreads=4)
    assert (st == 0).all() and (stb == 0).all()
    assert np.max(np.abs(y - d["y_out"]) / np.abs(d["y_out"]).max(axis=(0, 1))) < 1e-5
    assert np.max(np.abs(g - d["grad_params"]) / np.abs(d["grad_params"]).max(axis=1, keepdims=True)) < 4e-6
    assert np.max(np.abs(-lam - d["grad_y0"]) / np.abs(d["grad_y0"]).max(axis=1, keepdims=True)) < 4e-6


def test_default_batch_solves_everywhere_in_the_oracle():
    """Every draw of the default batch at B = 300 returns status 0, forward and backward, at rtol = atol = 1e-8 (the
    GPU tests compare this batch bit for bit), and stays clear of the pole of Gamma(1 - b x)."""
    from tools.problems import gamma_delay_batch
    d = gamma_delay_batch(300)
    orc = make_oracle("gamma_delay")
    cfg = orc.config(rtol=1e-8, atol=1e-8, rtolB=1e-8, atolB=1e-8, rtolQB=1e-8, atolQB=1e-8)
    tv = d["tvals"]
    y, st, _ = orc.solve_forward(cfg, d["y0"], d["ps"], d["pr"], 0.0, tv, nthreads=4)
    g, lam, stb, _ = orc.solve_backward(cfg, tv[-1], 0.0, tv, d["grads"], nthreads=4)
    assert (st == 0).all() and (stb == 0).all()
    assert np.isfinite(g).all() and np.isfinite(lam).all()
    assert (d["ps"][:, 2:3] * y[:, :, 0]).max() < 0.75
