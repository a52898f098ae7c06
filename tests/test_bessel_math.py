"""Bessel functions J, Y, I, K of integer order in generated right-hand sides -- the CPU half.

* ``csrc/sa_math_bessel.h`` (the fourth block of the math library, embedded after ``csrc/sa_math.h`` and the other
  blocks into the headers that call one of its functions): accuracy against mpmath at 200 bits for the orders 0, 1, 2,
  5 and ``SAM_BESSEL_NMAX``, special values, both sides of every piece boundary and of the switch of J's recurrence,
  the Wronskian identities.  Units: I and K in ulp of the result; J and Y in ulp of the result below the function's
  first zero and in units of spacing(M_n(x)), M_n = sqrt(J_n^2 + Y_n^2), beyond it.  Ceilings: 4 for the orders 0 and
  1 (the ceiling of the gamma block); for a higher order, per function and range, the worst value measured over this
  file's sample times 1.5, rounded up to an integer (``HIGHER_ORDER_CEILING``; the margin is for samples larger than
  this one);
* the code generator: besselj / bessely / besseli / besselk of an integer literal order are printed as
  ``sa_bessel_*`` calls; other orders raise; models without them keep their header byte for byte (sha256 of
  ``native_source()`` recorded on the parent commit);
* the callbacks of ``mathfn_f`` and ``bessel_ring`` against hand-written closed forms (mpmath, 40 digits; Bessel
  derivative identities written out here, nothing of sympy's differentiation or of the printers on that side);
* the oracle on ``bessel_ring`` against DOP853 truth (tools/make_golden_truth.py --bessel).

The GPU half (device == oracle bit for bit, device vs truth) is tests/test_gpu_bessel.py.
"""
import ctypes
import functools
import hashlib
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests.family_checks import compile_math_blocks
from tests.helpers import make_oracle, make_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ["j", "y", "i", "k"]
NMAX = 9
ORDERS = (0, 1, 2, 5, NMAX)
ULP_CEILING = 4.0                       # orders 0 and 1
N_POINTS = 1500
BELOW = "U(0,50) below the first zero"
#: orders >= 2: {(family, range): ceiling} = ceil(1.5 * the worst value measured over the sample of ``_ranges()`` for the
#: orders 2, 5 and 9 (the measured values stand in the header comment of csrc/sa_math_bessel.h); for J and Y the range
#: (0, 50) is split at the first zero of the function: below it the unit is the ulp of a result that vanishes at the zero
#: (single points next to it give the large figures), beyond it the ulp of the envelope
HIGHER_ORDER_CEILING = {
    ("j", "10^U(-300,0)"): 5, ("j", BELOW): 113, ("j", "U(0,50)"): 6, ("j", "U(50,1e6)"): 4, ("j", "U(1e6,2^50)"): 4,
    ("y", "10^U(-300,0)"): 13, ("y", BELOW): 661, ("y", "U(0,50)"): 5, ("y", "U(50,1e6)"): 5, ("y", "U(1e6,2^50)"): 4,
    ("i", "10^U(-300,0)"): 5, ("i", "U(0,30)"): 14, ("i", "U(30,713)"): 6,
    ("k", "10^U(-300,0)"): 13, ("k", "U(0,30)"): 10, ("k", "U(30,745)"): 6,
}


@pytest.fixture(scope="module")
def mathlib():
    """sa_math.h + sa_math_bessel.h compiled for the host exactly like the oracle compiles a generated header;
    ``call(family, order, x)``."""
    L = compile_math_blocks(("core", "bessel"), [
        "void w_%s(int n, int order, const double *x, double *o) "
        "{ for (int i = 0; i < n; i++) o[i] = sa_bessel_%s(order, x[i]); }" % (f, f) for f in FAMILIES])

    def call(name, order, x):
        x = np.ascontiguousarray(x, float)
        o = np.empty_like(x)
        getattr(L, "w_" + name)(len(x), int(order), ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(o.ctypes.data))
        return o
    return call


def _mp():
    import mpmath as mp
    mp.mp.prec = 200
    return mp


def _k_limit(n, x):
    """K_n(x) for n = 0, 1 as the limit pi/2 (I_-v - I_v) / sin(pi v), averaged over v = n +- 1e-40 at the precision
    the cancellation needs: mpmath's own besselk takes a third of a second per value for 2 < x < 60 (checked against
    it at a few points in test_reference_of_k)."""
    mp = _mp()
    with mp.workprec(200 + 2 * 140 + int(3 * float(x)) + 60):
        d = mp.mpf(10) ** -40

        def kv(v):
            return mp.pi / 2 * (mp.besseli(-v, x) - mp.besseli(v, x)) / mp.sin(v * mp.pi)
        r = (kv(n + d) + kv(n - d)) / 2
    return +r


def _upward(f0, f1, x, sign):
    """f_(k+1) = (2k/x) f_k + sign f_(k-1) up to the order NMAX + 1, at 200 bits (Y: sign -1, K: sign +1 -- the stable
    direction of both)"""
    out = [f0, f1]
    for k in range(1, NMAX + 1):
        out.append(2 * k / x * out[k] + sign * out[k - 1])
    return out


@functools.lru_cache(maxsize=None)
def _y_all(xf):
    mp = _mp()
    x = mp.mpf(xf)
    return _upward(mp.bessely(0, x), mp.bessely(1, x), x, -1)


@functools.lru_cache(maxsize=None)
def _k_all(xf):
    mp = _mp()
    x = mp.mpf(xf)
    if xf > 60:
        return _upward(mp.besselk(0, x), mp.besselk(1, x), x, 1)
    return _upward(_k_limit(0, x), _k_limit(1, x), x, 1)


@functools.lru_cache(maxsize=None)
def _true(name, n, xf):
    """The function at 200 bits: mpmath's besselj / besseli; Y and K of every order from mpmath's orders 0 and 1 by the
    upward recurrence (one pair of evaluations serves all orders of a point)."""
    mp = _mp()
    if name == "j":
        return mp.besselj(n, mp.mpf(xf))
    if name == "i":
        return mp.besseli(n, mp.mpf(xf))
    if xf < 0:
        return mp.nan
    return (_y_all(xf) if name == "y" else _k_all(xf))[n]


def _first_zero(name, n):
    """The first positive zero of J_n / Y_n."""
    mp = _mp()
    if (name, n) not in _FIRST_ZERO:
        _FIRST_ZERO[name, n] = float(mp.besseljzero(n, 1) if name == "j" else mp.besselyzero(n, 1))
    return _FIRST_ZERO[name, n]


_FIRST_ZERO = {}


def _unit(name, n, xv, r):
    """The unit the error at x is counted in: spacing(|f(x)|); for J and Y beyond the first zero spacing(M_n(x)),
    M_n = sqrt(J_n^2 + Y_n^2)."""
    mp = _mp()
    size = abs(float(r))
    xf = abs(float(xv))
    if name in "jy" and xf >= _first_zero(name, n):
        size = float(mp.sqrt(_true("j", n, xf) ** 2 + _true("y", n, xf) ** 2))
    return size


def _errors(name, n, x, got):
    """Errors of ``got`` against mpmath in the units of ``_unit``; a true value beyond the range of a double wants the
    infinity (or the zero) of its sign."""
    mp = _mp()
    out = []
    for xv, g in zip(x, got):
        xf = float(xv)
        r = _true(name, n, abs(xf)) * (-1 if (xf < 0 and n % 2) else 1) if name in "ji" else _true(name, n, xf)
        rf = float(r)
        if not np.isfinite(rf) or rf == 0.0:
            assert g == rf, (name, n, xv, g, rf)
            out.append(0.0)
            continue
        assert np.isfinite(g), (name, n, xv, g)
        out.append(float(abs(mp.mpf(float(g)) - r) / np.spacing(_unit(name, n, xv, r))))
    return np.array(out)


def test_reference_of_k():
    """The limit form the reference of K uses below 60 is mpmath's besselk."""
    mp = _mp()
    for xv in (1e-3, 0.7, 3.0, 25.0, 59.0):
        for n in (0, 1):
            assert abs(_k_limit(n, mp.mpf(xv)) / mp.besselk(n, mp.mpf(xv)) - 1) < mp.mpf(2) ** -190


def _ranges():
    """{family: {range: points}}: the ranges of the issue, 1 500 seeded points each."""
    rng = np.random.RandomState(0)
    N = N_POINTS
    osc = {"10^U(-300,0)": 10.0 ** rng.uniform(-300, 0, N), "U(0,50)": rng.uniform(0, 50, N),
           "U(50,1e6)": rng.uniform(50, 1e6, N), "U(1e6,2^50)": rng.uniform(1e6, 2.0 ** 50, N)}
    return {"j": osc, "y": osc,
            "i": {"10^U(-300,0)": 10.0 ** rng.uniform(-300, 0, N), "U(0,30)": rng.uniform(0, 30, N),
                  "U(30,713)": rng.uniform(30, 713, N)},
            "k": {"10^U(-300,0)": 10.0 ** rng.uniform(-300, 0, N), "U(0,30)": rng.uniform(0, 30, N),
                  "U(30,745)": rng.uniform(30, 745, N)}}


def _ceiling(name, n, label):
    return ULP_CEILING if n <= 1 else float(HIGHER_ORDER_CEILING[name, label])


def _label_of(name, x, n=0):
    """the range of ``_ranges()`` a point belongs to (for the ceiling of a higher order); J_n and Y_n, n >= 2: (0, 50)
    is split at the function's first zero, where the unit changes from the ulp of the result to that of the envelope"""
    x = abs(float(x))
    if name in "jy":
        if n >= 2 and 1 <= x < min(50.0, _first_zero(name, n)):
            return BELOW
        return "10^U(-300,0)" if x < 1 else ("U(0,50)" if x < 50 else ("U(50,1e6)" if x < 1e6 else "U(1e6,2^50)"))
    return "10^U(-300,0)" if x < 1 else ("U(0,30)" if x < 30 else ("U(30,713)" if name == "i" else "U(30,745)"))


@pytest.mark.parametrize("name", FAMILIES)
def test_accuracy_against_mpmath(mathlib, name):
    """Every order of ORDERS over the ranges of the issue: within the ceiling of its range; the measured worst cases
    are printed (the header comment carries them)."""
    worst = {}
    for label, x in _ranges()[name].items():
        for n in ORDERS:
            err = _errors(name, n, x, mathlib(name, n, x))
            if name in "jy" and label == "U(0,50)" and n >= 2:      # split at the first zero of the function
                below = x < _first_zero(name, n)
                worst[BELOW, n] = err[below].max()
                err = err[~below]
            worst[label, n] = err.max()
    for (label, n), w in worst.items():
        print("worst error %s_%d %-30s %.2f (ceiling %.0f)" % (name, n, label, w, _ceiling(name, n, label)))
    for (label, n), w in worst.items():
        assert w <= _ceiling(name, n, label), (name, n, label, w)
    for label in {lab for lab, _ in worst}:      # the ceilings of the higher orders are what the rule gives, no more
        assert HIGHER_ORDER_CEILING[name, label] == np.ceil(1.5 * max(worst[label, n] for n in ORDERS
                                                                      if n >= 2 and (label, n) in worst)), label


def test_special_values(mathlib):
    inf, nan = np.inf, np.nan

    def same(got, want):
        """equal values AND equal signs of zero; NaN where NaN is wanted"""
        got, want = np.asarray(got), np.asarray(want, float)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(np.signbit(got)[~np.isnan(want)], np.signbit(want)[~np.isnan(want)])
    for n in ORDERS + (4, 8):
        odd = n % 2 == 1
        # NaN, +-0, +-inf
        same(mathlib("j", n, [nan, 0.0, -0.0, inf, -inf]), [nan, 1.0, 1.0, 0.0, 0.0] if n == 0 else
             [nan, 0.0, -0.0 if odd else 0.0, 0.0, -0.0 if odd else 0.0])
        same(mathlib("i", n, [nan, 0.0, -0.0, inf, -inf]), [nan, 1.0, 1.0, inf, inf] if n == 0 else
             [nan, 0.0, -0.0 if odd else 0.0, inf, -inf if odd else inf])
        same(mathlib("y", n, [nan, 0.0, -0.0, inf, -inf, -1.0, -1e-300, -1e300]), [nan, -inf, -inf, 0.0, nan, nan, nan, nan])
        same(mathlib("k", n, [nan, 0.0, -0.0, inf, -inf, -1.0, -1e-300, -1e300]), [nan, inf, inf, 0.0, nan, nan, nan, nan])
        # parity on the negative axis, exactly
        x = np.array([1e-300, 1e-5, 0.3, 0.99, 1.0, 1.7, 2.5, 4.9, 7.0, 8.0, 9.0, 12.5, 40.0, 77.7, 300.0, 700.5, 1e5, 2.0 ** 50])
        sign = -1.0 if odd else 1.0
        same(mathlib("j", n, -x), sign * mathlib("j", n, x))
        same(mathlib("i", n, -x), sign * mathlib("i", n, x))
        # beyond the domain of sa_sin: NaN, as sa_sin; I's overflow, K's underflow
        same(mathlib("j", n, [2.0 ** 50 * 1.5, -1e300]), [nan, nan])
        same(mathlib("y", n, [2.0 ** 50 * 1.5, 1e300]), [nan, nan])
        same(mathlib("i", n, [720.0, 1e4, 1e300, -720.0]), [inf, inf, inf, -inf if odd else inf])
        same(mathlib("k", n, [760.0, 1e4, 1e300]), [0.0, 0.0, 0.0])
        assert np.isfinite(mathlib("j", n, [2.0 ** 50])[0]) and np.isfinite(mathlib("y", n, [2.0 ** 50])[0])
    # towards 0 the orders >= 1 of Y and K overflow to the infinity of their sign
    same(mathlib("y", 5, [1e-300, 1e-80, 5e-324]), [-inf, -inf, -inf])
    same(mathlib("k", 5, [1e-300, 1e-80, 5e-324]), [inf, inf, inf])
    same(mathlib("y", 1, [5e-324]), [-inf])
    same(mathlib("k", 1, [5e-324]), [inf])
    # I reaches its own overflow threshold, beyond exp's (709.78): I_0(713.9) is finite, I_0(714) is not
    got = mathlib("i", 0, [713.9, 713.98, 714.0])
    assert np.isfinite(got[:2]).all() and got[1] > 1.7e308 and got[2] == inf
    # K's last values before its underflow are subnormal, not zero
    got = mathlib("k", 0, [738.0, 741.0])
    assert (got > 0).all() and (got < 2.3e-308).all()


def _neighbours(b, k=1):
    x = [b]
    for _ in range(k):
        x = [np.nextafter(x[0], -np.inf)] + x + [np.nextafter(x[-1], np.inf)]
    return np.array(x)


def _check_around(mathlib, name, n, b):
    """nextafter(b, -inf), b, nextafter(b, +inf): each within the ceiling, and the three values differ from each other
    by no more than the ceiling plus the function's true change."""
    mp = _mp()
    x = _neighbours(b)
    got = mathlib(name, n, x)
    ceil = _ceiling(name, n, _label_of(name, b, n))
    err = _errors(name, n, x, got)
    assert (err <= ceil).all(), (name, n, b, err)
    true = [_true(name, n, float(v)) for v in x]
    unit = max(np.spacing(_unit(name, n, v, r)) for v, r in zip(x, true))
    for i in range(3):
        for j in range(i):
            change = abs(float(true[i] - true[j]))
            assert abs(got[i] - got[j]) <= ceil * unit + change, (name, n, b, got, change)


def test_both_sides_of_every_piece_boundary(mathlib):
    """The boundaries come from the header's own definitions (codegen.math_boundaries("bessel"))."""
    from sunode_amd.symode import codegen
    bounds = codegen.math_boundaries("bessel")
    assert set(bounds) == {"j0", "j1", "y0", "y1", "i0", "i1", "k0", "k1", "jn", "in"}
    assert len(bounds["j0"]) == 4 and len(bounds["y0"]) == 6 and len(bounds["i0"]) == 3 and len(bounds["k0"]) == 5
    assert len(bounds["in"]) == 3 and len(bounds["jn"]) == 1
    for key, bs in bounds.items():
        name = key[0]
        orders = (int(key[1]),) if key[1] in "01" else (2, 5, NMAX)
        for b in bs:
            for n in orders:
                _check_around(mathlib, name, n, b)
    # every order goes through the pieces of the orders 0 and 1 as well (Y, K upwards from them; J from |x| = n on;
    # I normalises by I0)
    for name in FAMILIES:
        for b in sorted(set(bounds[name + "0"]) | set(bounds[name + "1"])):
            for n in (2, 5, NMAX):
                _check_around(mathlib, name, n, b)


def test_both_sides_of_the_switch_of_the_recurrence_of_j(mathlib):
    """J_n runs downwards (Miller) below |x| = n and upwards from there on."""
    for n in (2, 5, NMAX):
        _check_around(mathlib, "j", n, float(n))
        x = np.concatenate([_neighbours(float(n), 8), n + np.array([-0.5, -1e-3, -1e-9, 1e-9, 1e-3, 0.5])])
        for v in (x, -x):
            assert (_errors("j", n, v, mathlib("j", n, v)) <= _ceiling("j", n, BELOW)).all(), n          # (n < the first zero)


def _away_from_zeros(mathlib, names, orders, x):
    """points at which none of the named functions is within 1e-3 (relative to its envelope) of a zero"""
    keep = np.ones(len(x), bool)
    for name in names:
        for n in orders:
            v = mathlib(name, n, x)
            env = np.sqrt(mathlib("j", n, x) ** 2 + mathlib("y", n, x) ** 2) if name in "jy" else np.abs(v)
            keep &= np.abs(v) >= 1e-3 * env
    return x[keep]


def test_wronskian_identities(mathlib):
    """J_(n+1) Y_n - J_n Y_(n+1) = 2 / (pi x) and I_n K_(n+1) + I_(n+1) K_n = 1 / x at 200 points each, to what the
    ceilings of the four factors allow: every factor carries its ceiling in its own unit (2^-52 of its value or of its
    envelope), the products and the sum three roundings more."""
    rng = np.random.RandomState(7)
    eps = 2.0 ** -52
    done = 0
    for n in (0, 1, 4, NMAX - 1):
        x = _away_from_zeros(mathlib, "jy", (n, n + 1), rng.uniform(0.3, 60.0, 80))[:50]
        assert len(x) == 50
        j0, j1, y0, y1 = (mathlib(f, k, x) for f, k in (("j", n), ("j", n + 1), ("y", n), ("y", n + 1)))
        for i, xv in enumerate(x):
            cj = [_ceiling("j", k, _label_of("j", xv, k)) for k in (n, n + 1)]
            cy = [_ceiling("y", k, _label_of("y", xv, k)) for k in (n, n + 1)]
            uj = [_unit("j", k, xv, v) for k, v in ((n, j0[i]), (n + 1, j1[i]))]
            uy = [_unit("y", k, xv, v) for k, v in ((n, y0[i]), (n + 1, y1[i]))]
            tol = eps * (cj[1] * uj[1] * abs(y0[i]) + cy[0] * uy[0] * abs(j1[i]) + cj[0] * uj[0] * abs(y1[i])
                         + cy[1] * uy[1] * abs(j0[i]) + 3 * (abs(j1[i] * y0[i]) + abs(j0[i] * y1[i])))
            assert abs((j1[i] * y0[i] - j0[i] * y1[i]) - 2 / (np.pi * xv)) <= tol, (n, xv)
            done += 1
    assert done == 200
    done = 0
    for n in (0, 1, 4, NMAX - 1):
        x = np.concatenate([10.0 ** rng.uniform(-2, 0, 10), rng.uniform(1.0, 300.0, 40)])
        i0, i1, k0, k1 = (mathlib(f, k, x) for f, k in (("i", n), ("i", n + 1), ("k", n), ("k", n + 1)))
        for i, xv in enumerate(x):
            ci = [_ceiling("i", k, _label_of("i", xv)) for k in (n, n + 1)]
            ck = [_ceiling("k", k, _label_of("k", xv)) for k in (n, n + 1)]
            tol = eps * ((ci[0] + ck[1] + 3) * i0[i] * k1[i] + (ci[1] + ck[0] + 3) * i1[i] * k0[i])
            assert abs((i0[i] * k1[i] + i1[i] * k0[i]) - 1 / xv) <= tol, (n, xv)
            done += 1
    assert done == 200


# ---- the code generator ----
NEW_MODELS = ("mathfn_f", "bessel_ring")


def _source(rhs, params={"a": ()}, states={"x": ()}, dparams=[("a",)]):
    from sunode_amd import SympyProblem
    return SympyProblem(params, states, rhs, dparams).native_source()


def test_printer_emits_the_calls_with_a_literal_order():
    import sympy as sym
    src = _source(lambda t, y, p: {"x": sym.besselj(2, p.a * y.x)})
    body = src.split("#endif /* SA_MATH_BESSEL_H */")[1]
    assert "sa_bessel_j(2, " in body
    assert "sa_bessel_j(1, " in body and "sa_bessel_j(3, " in body          # the derivative: (J1 - J3) / 2
    for fn, letter in ((sym.bessely, "y"), (sym.besseli, "i"), (sym.besselk, "k")):
        body = _source(lambda t, y, p: {"x": fn(2, p.a * y.x)}).split("#endif /* SA_MATH_BESSEL_H */")[1]
        assert "sa_bessel_%s(2, " % letter in body


def test_negative_integer_orders_build():
    import sympy as sym
    from sunode_amd.symode.codegen import HipExprPrinter
    src = _source(lambda t, y, p: {"x": sym.besselj(-1, p.a * y.x) + sym.besselk(-2, 1 + y.x * y.x)})
    body = src.split("#endif /* SA_MATH_BESSEL_H */")[1]
    assert "sa_bessel_j(1, " in body and "sa_bessel_k(2, " in body
    # what sympy leaves of a negative literal goes through the reflection identities
    u = sym.Symbol("u")
    pr = HipExprPrinter({})
    raw = {f: f(-3, u, evaluate=False) for f in (sym.besselj, sym.bessely, sym.besseli, sym.besselk)}
    assert pr.doprint(raw[sym.besselj]) == "(-sa_bessel_j(3, u))" and pr.doprint(raw[sym.bessely]) == "(-sa_bessel_y(3, u))"
    assert pr.doprint(raw[sym.besseli]) == "sa_bessel_i(3, u)" and pr.doprint(raw[sym.besselk]) == "sa_bessel_k(3, u)"
    assert pr.doprint(sym.besselj(-2, u, evaluate=False)) == "sa_bessel_j(2, u)"


def test_other_orders_raise():
    import sympy as sym
    from sunode_amd.symode import codegen
    assert codegen.math_bessel_nmax() == NMAX
    nu = sym.Symbol("nu")
    for order in (sym.Rational(1, 2), nu, NMAX + 1, 2.0):
        for fn in (sym.besselj, sym.bessely, sym.besseli, sym.besselk):
            with pytest.raises(NotImplementedError, match="SAM_BESSEL_NMAX = %d" % NMAX):
                _source(lambda t, y, p: {"x": -p.a * y.x + fn(order, 1 + y.x * y.x)})
    # the order NMAX itself needs NMAX + 1 for the derivative of a state: in a forcing of t alone it builds
    src = _source(lambda t, y, p: {"x": -p.a * y.x + sym.besselj(NMAX, t)})
    assert "sa_bessel_j(%d, " % NMAX in src
    src = _source(lambda t, y, p: {"x": sym.besselk(NMAX - 1, p.a * y.x)})
    assert "sa_bessel_k(%d, " % NMAX in src


def test_new_models_build_without_a_warning_and_call_the_deterministic_functions_only():
    """(``SympyProblem`` of a Bessel model: PrintMethodNotImplementedError on the parent commit)"""
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
        assert "SA_HAVE_MATH_BESSEL" in src and "SA_HAVE_MATH_INV" not in src and "SA_HAVE_MATH_GAMMA" not in src
        assert src.index("#endif /* SA_MATH_H */") < src.index("#ifndef SA_MATH_BESSEL_H")
        body = src.split("#endif /* SA_MATH_BESSEL_H */")[1]
        for fn in FAMILIES:
            assert "sa_bessel_%s(" % fn in body, (name, fn)
    body = make_problem("mathfn_f").native_source().split("#endif /* SA_MATH_BESSEL_H */")[1]
    rhs = body[body.index("sa_rhs"):body.index("sa_jac")]
    assert "sa_bessel_i(2, " in rhs and "sa_bessel_j(2, " in rhs                      # an order >= 2 directly
    assert "sa_bessel_j(3, " in body and "sa_bessel_j(3, " not in rhs                  # ... and one through a derivative only
    assert "sa_bessel_i(3, " in body and "sa_bessel_i(3, " not in rhs


def test_the_block_comes_after_the_other_blocks():
    import sympy as sym
    src = _source(lambda t, y, p: {"x": sym.atan(y.x) - p.a * sym.loggamma(1 + y.x * y.x) + sym.besselj(0, t)})
    assert (src.index("#endif /* SA_MATH_H */") < src.index("#endif /* SA_MATH_INV_H */")
            < src.index("#endif /* SA_MATH_GAMMA_H */") < src.index("#ifndef SA_MATH_BESSEL_H"))


def test_existing_headers_keep_their_text(golden_dir):
    with open(os.path.join(golden_dir, "native_source_sha256.json")) as fh:
        digests = json.load(fh)
    for name in ("lv", "misc", "forcing", "logistic_switch", "mathfn_a", "mathfn_c", "mathfn_e", "probit_gate", "gamma_delay"):
        src = make_problem(name).native_source()
        assert "SA_HAVE_MATH_BESSEL" not in src
        assert hashlib.sha256(src.encode()).hexdigest() == digests[name], name


def test_host_helpers_agree_with_scipy():
    """``HOST_FUNCTIONS`` (sympy.lambdify of a model's expressions on the host) knows the four names: 50 points."""
    import sympy as sym
    from scipy import special
    from sunode_amd.symode.problem import HOST_FUNCTIONS
    u = sym.Symbol("u")
    expr = [sym.besselj(0, u), sym.besselj(3, u), sym.bessely(1, u), sym.besseli(2, u), sym.besselk(0, u), sym.besselk(4, u)]
    fn = sym.lambdify([u], expr, modules=[HOST_FUNCTIONS, "numpy"])
    for v in np.random.RandomState(2).uniform(0.05, 30.0, 50):
        want = [special.jv(0, v), special.jv(3, v), special.yv(1, v), special.iv(2, v), special.kv(0, v), special.kv(4, v)]
        np.testing.assert_allclose(np.asarray(fn(v), float), want, rtol=1e-14)


def test_generator_reproduces_the_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_sa_math_coeffs.py"), "--check", "--bessel"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- the callbacks against closed forms ----
def _mathfn_f_closed_forms(x, a, lam):
    """Values f_i(x_i, a_i) of ``mathfn_f`` and their partial derivatives, written by hand (mpmath): J0' = -J1,
    K0' = -K1, Y1' = Y0 - Y1/u, K1' = -K0 - K1/u, I2' = I1 - 2 I2/u, J2' = J1 - 2 J2/u."""
    import mpmath as mp
    x = [mp.mpf(float(v)) for v in x]
    a = [mp.mpf(float(v)) for v in a]
    J, Y, I, K = mp.besselj, mp.bessely, mp.besseli, mp.besselk
    u = [a[0] * x[0], x[1] / a[1], a[2] * x[2], a[3] * x[3], x[4] / a[4]]
    v3 = x[3] / a[3]
    d = [-J(1, u[0]), Y(0, u[1]) - Y(1, u[1]) / u[1], I(1, u[2]) - 2 * I(2, u[2]) / u[2], -K(1, u[3]),
         -K(0, u[4]) - K(1, u[4]) / u[4]]
    dv3 = J(1, v3) - 2 * J(2, v3) / v3
    f = [J(0, u[0]), Y(1, u[1]), I(2, u[2]), K(0, u[3]) + J(2, v3), K(1, u[4])]
    fx = [a[0] * d[0], d[1] / a[1], a[2] * d[2], a[3] * d[3] + dv3 / a[3], d[4] / a[4]]
    fa = [x[0] * d[0], -x[1] / a[1] ** 2 * d[1], x[2] * d[2], x[3] * d[3] - x[3] / a[3] ** 2 * dv3, -x[4] / a[4] ** 2 * d[4]]
    n = 5
    Jm = np.zeros((n, n))
    Jm[np.arange(n), np.arange(n)] = [float(v) for v in fx]          # f_i depends on x_i and a_i only
    fa = np.array([float(v) for v in fa])
    return dict(rhs=np.array([float(v) for v in f]), jac=Jm, adj=-lam @ Jm, quad=lam * fa, adjjac=-Jm.T)


def _bessel_ring_closed_forms(t, y, ps, pr, lam):
    """``bessel_ring`` by hand: R = I1/I0 has R' = 1 - R/u - R^2; J0' = -J1, K0' = -K1, Y0' = -Y1, Y1' = Y0 - Y1/s."""
    import mpmath as mp
    t = mp.mpf(float(t))
    x, z, c = [mp.mpf(float(v)) for v in y]
    b, w, g, A, kappa = [mp.mpf(float(v)) for v in ps]
    m, e, d, q, r = [mp.mpf(float(v)) for v in pr]
    u = b * x
    R = mp.besseli(1, u) / mp.besseli(0, u)
    dR = 1 - R / u - R * R
    s = 1 + x - z
    v = kappa + z * z
    f = [A * R - m * x + e * mp.besselj(0, w * t), g * x - d * z + q * mp.besselk(0, v) - r * mp.bessely(1, s),
         mp.bessely(0, s) / 5 - c / 5]
    Jm = np.zeros((3, 3))
    Jm[0, 0] = float(A * b * dR - m)
    dY1 = mp.bessely(0, s) - mp.bessely(1, s) / s
    Jm[1, 0] = float(g - r * dY1)
    Jm[1, 1] = float(-d - 2 * z * q * mp.besselk(1, v) + r * dY1)
    Jm[2, 0] = float(-mp.bessely(1, s) / 5)
    Jm[2, 1] = float(mp.bessely(1, s) / 5)
    Jm[2, 2] = -0.2
    P = np.zeros((3, 5))                                             # d f_i / d (b, w, g, A, kappa)
    P[0, 0] = float(A * x * dR)
    P[0, 1] = float(-e * t * mp.besselj(1, w * t))
    P[0, 3] = float(R)
    P[1, 2] = float(x)
    P[1, 4] = float(-q * mp.besselk(1, v))
    return dict(rhs=np.array([float(v) for v in f]), jac=Jm, adj=-lam @ Jm, quad=lam @ P, adjjac=-Jm.T)


def _compare(got, want, n):
    """rtol 1e-13 of the row maximum (of the whole vector for rhs / adj / quad)"""
    for key in ("rhs", "jac", "adj", "quad", "adjjac"):
        g = np.asarray(got[key], float)
        w = want[key]
        if key in ("jac", "adjjac"):
            g = g.reshape(n, n, order="F")
            scale = np.abs(w).max(axis=1, keepdims=True)
        else:
            scale = np.abs(w).max()
        assert (np.abs(g - w) <= 1e-13 * scale).all(), (key, g, w)


def test_callbacks_against_hand_written_closed_forms():
    """32 points each: the oracle's five callbacks of ``mathfn_f`` and ``bessel_ring`` against closed forms of the
    values and first derivatives.  The arguments of ``mathfn_f`` stay in (0.18, 2), below the first zeros of J1, J2 and
    Y1, where every entry is accurate relative to itself."""
    import mpmath as mp
    mp.mp.dps = 40
    orc = make_oracle("mathfn_f")
    rng = np.random.RandomState(3)
    for _ in range(32):
        x = rng.uniform(0.2, 1.8, 5)
        a = rng.uniform(1.02, 1.1, 5)
        lam = rng.randn(5)
        got = orc.eval(0.0, x, lam, a, np.zeros(0))
        assert np.asarray(got["codes"]).tolist() == [0] * 5
        _compare(got, _mathfn_f_closed_forms(x, a, lam), 5)
    orc = make_oracle("bessel_ring")
    for _ in range(32):
        t = rng.uniform(0.0, 8.0)
        y = np.array([rng.uniform(0.05, 2.0), rng.uniform(0.0, 0.9), rng.uniform(-1.0, 1.0)])
        ps = np.array([2.0, 1.5, 0.3, 1.0, 0.5]) * np.exp(0.2 * rng.randn(5))
        pr = np.array([0.5, 0.3, 0.6, 0.2, 0.05])
        lam = rng.randn(3)
        got = orc.eval(t, y, lam, ps, pr)
        assert np.asarray(got["codes"]).tolist() == [0] * 5
        _compare(got, _bessel_ring_closed_forms(t, y, ps, pr, lam), 3)


# ---- the integrated model ----
def test_truth_draws_cross_piece_boundaries_and_a_zero_of_j0(golden_dir):
    """Along each of the 16 truth draws the argument w t of the forcing J0(w t) crosses at least two piece boundaries
    of J0 and at least one of its zeros; the argument of K0 stays strictly positive, that of Y0 as well."""
    from sunode_amd.symode import codegen
    d = np.load(os.path.join(golden_dir, "truth_bessel_ring.npz"))
    assert d["y0"].shape[0] == 16
    bounds = np.array(codegen.math_boundaries("bessel")["j0"])
    zeros = np.array([2.404825557695773, 5.520078110286311, 8.653727912911013])
    for i in range(16):
        lo, hi = d["ps"][i, 1] * d["tvals"][0], d["ps"][i, 1] * d["tvals"][-1]
        assert ((bounds > lo) & (bounds < hi)).sum() >= 2 and ((zeros > lo) & (zeros < hi)).sum() >= 1
        x, z = d["y_out"][i, :, 0], d["y_out"][i, :, 1]
        assert (1 + x - z).min() > 0.5 and (d["ps"][i, 4] + z * z).min() > 0.2


def test_oracle_forward_adjoint_matches_truth_on_bessel_ring(golden_dir):
    """The bars of tests/test_gpu_transcendental.py at rtol = atol = 1e-8: states <= 1e-5, gradients and -lamda <= 4e-6
    relative to the per-draw maximum, against DOP853 truth (16 draws)."""
    d = np.load(os.path.join(golden_dir, "truth_bessel_ring.npz"))
    orc = make_oracle("bessel_ring")
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
    GPU tests compare this batch bit for bit), and keeps the argument of Y0 away from zero."""
    from tools.problems import bessel_ring_batch
    d = bessel_ring_batch(300)
    orc = make_oracle("bessel_ring")
    cfg = orc.config(rtol=1e-8, atol=1e-8, rtolB=1e-8, atolB=1e-8, rtolQB=1e-8, atolQB=1e-8)
    tv = d["tvals"]
    y, st, _ = orc.solve_forward(cfg, d["y0"], d["ps"], d["pr"], 0.0, tv, nthreads=4)
    g, lam, stb, _ = orc.solve_backward(cfg, tv[-1], 0.0, tv, d["grads"], nthreads=4)
    assert (st == 0).all() and (stb == 0).all()
    assert np.isfinite(g).all() and np.isfinite(lam).all()
    assert (1 + y[:, :, 0] - y[:, :, 1]).min() > 0.5
