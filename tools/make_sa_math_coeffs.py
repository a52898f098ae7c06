"""Coefficients of sunode_amd/csrc/sa_math_inv.h (inverse trigonometric / hyperbolic functions, erf, erfc), of
sunode_amd/csrc/sa_math_gamma.h (lgamma, tgamma, digamma, trigamma) and of sunode_amd/csrc/sa_math_bessel.h (J, Y, I, K
of the orders 0 and 1).

Every polynomial of that header is a Chebyshev-node interpolant (near-minimax) computed here with mpmath at 120
digits, converted to the monomial basis of the header's own variable, rounded to double and then MEASURED: the
error of the rounded polynomial against the function, in exact arithmetic, over 1 001 points of the fit
interval (201 points for sa_math_bessel.h, whose functions are expensive at that precision).  Nothing is transcribed from another library.

    python tools/make_sa_math_coeffs.py            # prints the literal blocks the headers carry
    python tools/make_sa_math_coeffs.py --check    # compares them with the headers' text (exit status 1 on a difference)
    python tools/make_sa_math_coeffs.py --gamma    # (with either form) only sa_math_gamma.h; --inv: only sa_math_inv.h;
                                                   # --bessel: only sa_math_bessel.h (its 50 fits run in parallel)

Sets (variable, interval, form):

  ATAN    P(z) = (t - atan t) / t^3,  z = t^2 in [0, (7/16)^2]          atan t = t - t z P(z)
  ASIN    Q(z) = (asin s - s) / s^3,  z = s^2 in [0, 1/4]               asin s = s + s z Q(z)
  ERF     one Horner chain whose coefficients are selected among the pieces below:
            piece 0   E(z) = erf(s)/s - 1,   z = s^2 in [0, 1]                      erf x = x + x E(x^2)
            piece i   X_i(w) = erfcx(c_i + w),  |w| <= h_i          (argument pieces, a = |x| in [c_i - h_i, c_i + h_i])
            piece j   A_j(w) = a erfcx(a), a = (u_j + w)^(-1/2)     (asymptotic pieces in u = 1/a^2)
          erfcx(a) = exp(a^2) erfc(a).

sa_math_gamma.h: one Horner chain per function, coefficients selected among four pieces (y: the argument, after the
shift x + 1 of a small one or the reflection 1 - x / -x of a negative one):

  LGAMMA    pieces 0-2  G(w) = lgamma(y) / ((y - 1)(y - 2)),  y = c_i + w in [3/4, 3/2], [3/2, 3], [3, 6]
            piece 3     S(w) = y (lgamma(y) - (y - 1/2) ln y + y - ln(2 pi)/2),  w = 1/y^2 in [0, 1/36]
                        (also the exponent of tgamma, whose argument an upward recurrence lifts to y >= 6)
  DIGAMMA   piece 0     psi(y) / (y - x0),  y = c_0 + w in [1, 2]  (x0: the positive root, carried in two words)
            pieces 1-2  psi(y),  y = c_i + w in [2, 4], [4, 8]
            piece 3     D(w) = (ln y - 1/(2y) - psi(y)) / w,  w = 1/y^2 in [0, 1/64]
  TRIGAMMA  pieces 0-2  psi'(y),  y = c_i + w in [1, 2], [2, 4], [4, 8]
            piece 3     T(w) = (y psi'(y) - 1 - 1/(2y)) / w,  w = 1/y^2 in [0, 1/64]

sa_math_bessel.h: one Horner chain per function of order 0 / 1, coefficients selected among the pieces of |x| (the
orders >= 2 are recurrences and series without fitted coefficients):

  J0, J1    pieces 0-2  J0(x) | J1(x)/x on [0, 1.5];  J(x) / (x - z) on the piece that holds the first zero z (two
                        words);  J(x) up to 8 (error relative to the modulus M = |H^(1)|), all in x - c
            pieces 3-4  P(1/x) on [8, 16], [16, inf) in 1/x - c;  J0Q, J1Q: Q(1/x) on the same pieces, where
                        H^(1)_n(x) = sqrt(2/(pi x)) (P + i Q) exp(i (x - n pi/2 - pi/4))
  Y0, Y1    pieces 1-4  Y(x) on [0.5, 1.25], [1.25, 2.5], [2.5, 5], [5, 8] in x - c, the first zero factored out of its
                        piece;  pieces 5-6: P as for J.  Y0S, Y1S: the polynomials A, B of x^2 on [0, 0.25] of
                        Y0 = ln x A + B, Y1 = x (ln x A + B) - (2/pi)/x
  I0, I1    piece 0     I0(x) | I1(x)/x in x^2 on [0, 64];  pieces 1-2: sqrt(x) exp(-x) I(x) in 1/x - c on [8, 16], [16, inf)
  K0, K1    pieces 1-5  sqrt(x) exp(x) K(x) in 1/x - c on [1, 2], [2, 4], [4, 8], [8, 16], [16, inf).  K0S, K1S: the
                        polynomials A, B of x^2 on [0, 1] of K0 = -ln x A + B, K1 = 1/x + x (ln x A + B)
"""
from __future__ import annotations

import os
import re
import sys

import mpmath as mp

mp.mp.dps = 120
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sunode_amd", "csrc", "sa_math_inv.h")
HEADER_GAMMA = os.path.join(os.path.dirname(HEADER), "sa_math_gamma.h")
HEADER_BESSEL = os.path.join(os.path.dirname(HEADER), "sa_math_bessel.h")

#: interval boundaries of atan's argument reduction (|x|): the header's SAM_ATAN_B1..4; the reduced argument is
#: largest, 7/16, at the upper end of the first interval
ATAN_BOUNDS = ("0.4375", "0.6875", "1.1875", "2.4375")
#: erf / erfc: |x| boundaries of the pieces (piece 0 below the first, the erfcx pieces between them): SAM_ERF_B1..5
ERF_BOUNDS = ("1.0", "1.5", "2.5", "4.0", "8.0")
#: erfc uses 1 - erf(x) for -1 < x < ERFC_DIRECT and the erfcx pieces from there on; the first erfcx piece therefore
#: starts at ERFC_DIRECT (SAM_ERFC_B1), not at ERF_BOUNDS[0]
ERFC_DIRECT = "0.5"
#: beyond this erfc underflows to zero (exp(-27.3^2) < 2^-1075): the argument is clamped here (SAM_ERFC_CLAMP)
ERFC_CLAMP = "27.5"
#: sa_math_gamma.h: boundaries of the pieces in y (SAM_LGAMMA_B1..4, SAM_DIGAMMA_B1..4, SAM_TRIGAMMA_B1..4); below the
#: first one the argument is shifted by one (lgamma x = lgamma(x + 1) - ln x, psi x = psi(x + 1) - 1/x, ...)
LGAMMA_BOUNDS = ("0.75", "1.5", "3.0", "6.0")
DIGAMMA_BOUNDS = ("1.0", "2.0", "4.0", "8.0")
TRIGAMMA_BOUNDS = ("1.0", "2.0", "4.0", "8.0")
#: error asked of every fit before its coefficients are rounded (relative to the quantity the header forms from it):
#: the rounding of the leading coefficient alone is up to 2^-54, the evaluation's roundings more
TARGET = mp.mpf(2) ** -58


def lit(x) -> str:
    return repr(float(x))


def fit(f, lo, hi, weight=None, target=TARGET, centred=False, nmin=4, nmax=40, npts=1000, stride=1):
    """Smallest-degree Chebyshev interpolant of f on [lo, hi] (monomial basis in x, or in x - (lo + hi)/2 when
    ``centred``) whose error, BEFORE its coefficients are rounded to double, is below ``target`` relative to
    ``weight(x)`` (default: |f(x)| itself) -- the size of the quantity the header forms from the polynomial.
    ``npts``: the error is measured at npts + 1 equidistant points.  ``stride`` > 1: the degrees are tried ``stride`` apart
    first and then downwards one by one from the first that passes (the same degree where the error falls with the
    degree; fewer evaluations of an expensive f).
    -> (double coefficients low..high, that error measured again AFTER the rounding, centre)."""
    lo, hi = mp.mpf(lo), mp.mpf(hi)
    c = (lo + hi) / 2 if centred else mp.mpf(0)
    g = (lambda w: f(c + w))
    a, b = lo - c, hi - c
    pts = [a + (b - a) * mp.mpf(k) / npts for k in range(npts + 1)]
    want = [g(w) for w in pts]
    scale = [abs(v) if weight is None else abs(weight(c + w)) for v, w in zip(want, pts)]

    def worst(poly):
        return max(abs(mp.polyval(poly, w) - v) / sc for w, v, sc in zip(pts, want, scale) if sc != 0)
    best = None
    for n in range(nmin, nmax, stride):
        coeffs = mp.chebyfit(g, [a, b], n)                       # highest power first
        if worst(coeffs) < target:
            best = coeffs
            for m in range(n - 1, max(n - stride, nmin - 1), -1):
                coeffs = mp.chebyfit(g, [a, b], m)
                if not worst(coeffs) < target:
                    break
                best = coeffs
            rounded = [mp.mpf(float(v)) for v in best]
            return [float(v) for v in rounded[::-1]], worst(rounded), c
    raise RuntimeError("no fit of degree < %d reaches %s" % (nmax, mp.nstr(target, 3)))


def f_atan(z):
    if z == 0:
        return mp.mpf(1) / 3
    t = mp.sqrt(z)
    return (t - mp.atan(t)) / (t * z)


def f_asin(z):
    if z == 0:
        return mp.mpf(1) / 6
    s = mp.sqrt(z)
    return (mp.asin(s) - s) / (s * z)


def f_erf(z):
    if z == 0:
        return 2 / mp.sqrt(mp.pi) - 1
    s = mp.sqrt(z)
    return mp.erf(s) / s - 1


def w_atan(z):            # (atan t / t) / z: the size of atan t in units of the term t z P(z)
    t = mp.sqrt(z)
    return mp.atan(t) / (t * z) if z != 0 else mp.mpf(0)


def w_asin(z):
    s = mp.sqrt(z)
    return mp.asin(s) / (s * z) if z != 0 else mp.mpf(0)


def w_erf(z):
    return mp.erf(mp.sqrt(z)) / mp.sqrt(z) if z != 0 else 2 / mp.sqrt(mp.pi)


def erfcx(a):
    return mp.exp(a * a) * mp.erfc(a)


def f_asym(u):
    a = 1 / mp.sqrt(u)
    return a * erfcx(a)


def horner(name, coeffs, var, indent="    "):
    lines = ["%sdouble %s = %s;" % (indent, name, lit(coeffs[-1]))]
    lines += ["%s%s = fma(%s, %s, %s);" % (indent, name, name, var, lit(v)) for v in coeffs[-2::-1]]
    return lines


def hi_lo(x):
    hi = mp.mpf(float(x))
    return lit(hi), lit(x - hi)


def blocks():
    out = {}
    # ---- constants: values as a double and what the double misses ----
    lines = []
    for name, value in (("ATAN_HALF", mp.atan(mp.mpf(1) / 2)), ("PIO4", mp.pi / 4), ("ATAN_3HALF", mp.atan(mp.mpf(3) / 2)),
                        ("PI", mp.pi)):
        hi, lo = hi_lo(value)
        lines += ["#define SAM_%s_HI %s" % (name, hi), "#define SAM_%s_LO %s" % (name, lo)]
    lines += ["#define SAM_3PIO4 %s" % lit(3 * mp.pi / 4), "#define SAM_LN2 %s" % lit(mp.log(2))]
    out["CONST"] = lines
    # ---- atan ----
    c, err, _ = fit(f_atan, 0, mp.mpf(7) / 16 * mp.mpf(7) / 16, weight=w_atan)
    out["ATAN"] = ["    /* P(z) = (t - atan t) / t^3, z = t^2 in [0, (7/16)^2]: degree %d, error 2^%.1f */"
                   % (len(c) - 1, float(mp.log(err, 2)))] + horner("p", c, "z")
    # ---- asin ----
    c, err, _ = fit(f_asin, 0, mp.mpf(1) / 4, weight=w_asin)
    out["ASIN"] = ["    /* Q(z) = (asin s - s) / s^3, z = s^2 in [0, 1/4]: degree %d, error 2^%.1f */"
                   % (len(c) - 1, float(mp.log(err, 2)))] + horner("q", c, "z")
    # ---- erf / erfc ----
    b = [mp.mpf(v) for v in ERF_BOUNDS]
    pieces = []                                                  # (description, coefficients low..high, centre text)
    c0, err, _ = fit(f_erf, 0, b[0] * b[0], weight=w_erf)
    pieces.append(("piece 0: E(z) = erf(s)/s - 1, z = s^2 in [0, %s]: degree %d, error 2^%.1f"
                   % (lit(b[0] * b[0]), len(c0) - 1, float(mp.log(err, 2))), c0, None))
    lows = [mp.mpf(ERFC_DIRECT)] + b[1:3]
    highs = b[1:4]
    for k, (lo, hi) in enumerate(zip(lows, highs)):
        ck, err, cen = fit(erfcx, lo, hi, centred=True)
        pieces.append(("piece %d: erfcx(c + w), c = %s, a in [%s, %s]: degree %d, error 2^%.1f"
                       % (k + 1, lit(cen), lit(lo), lit(hi), len(ck) - 1, float(mp.log(err, 2))), ck, lit(cen)))
    edges = [b[3], b[4], mp.mpf(ERFC_CLAMP)]
    for k in range(2):
        ulo, uhi = 1 / (edges[k + 1] ** 2), 1 / (edges[k] ** 2)
        cen = mp.mpf(float((ulo + uhi) / 2))
        half = max(uhi - cen, cen - ulo)
        ck, err, _ = fit(lambda w, cen=cen: f_asym(cen + w), -half, half)
        pieces.append(("piece %d: a erfcx(a) at 1/a^2 = c + w, c = %s, a in [%s, %s]: degree %d, error 2^%.1f"
                       % (k + 4, lit(cen), lit(edges[k]), lit(edges[k + 1]), len(ck) - 1, float(mp.log(err, 2))), ck, lit(cen)))
    deg = max(len(p[1]) for p in pieces) - 1
    lines = ["    /* coefficients by piece (zero above a piece's own degree); one Horner chain of degree %d" % deg]
    lines += ["       %s" % p[0] for p in pieces]
    lines[-1] += " */"
    for k, p in enumerate(pieces):
        if p[2] is not None:
            lines.append("#define SAM_ERF_C%d %s" % (k, p[2]))

    def sel(j):
        return "SAM_ERF_SEL(%s)" % ", ".join(lit(p[1][j]) if j < len(p[1]) else "0.0" for p in pieces)
    lines.append("#define SAM_ERF_HORNER(p, w) \\")
    lines.append("    p = %s; \\" % sel(deg))
    for j in range(deg - 1, -1, -1):
        lines.append("    p = fma(p, w, %s);%s" % (sel(j), " \\" if j else ""))
    out["ERF"] = lines
    return out


# ---- sa_math_gamma.h ----
def psi_root():
    return mp.findroot(lambda v: mp.psi(0, v), mp.mpf("1.4616321449683623"))


def f_lgamma(y):
    """lgamma(y) / ((y - 1)(y - 2)): gamma_E at 1 and 1 - gamma_E at 2"""
    d = (y - 1) * (y - 2)
    if abs(d) < mp.mpf(10) ** -60:
        return mp.euler if abs(y - 1) < 0.5 else 1 - mp.euler
    return mp.loggamma(y) / d


def f_stirling(w):
    if w == 0:
        return mp.mpf(1) / 12
    y = 1 / mp.sqrt(w)
    return y * (mp.loggamma(y) - (y - mp.mpf(1) / 2) * mp.log(y) + y - mp.log(2 * mp.pi) / 2)


def f_digamma0(y):
    x0 = psi_root()
    if abs(y - x0) < mp.mpf(10) ** -60:
        return mp.psi(1, x0)
    return mp.psi(0, y) / (y - x0)


def f_digamma_asym(w):
    if w == 0:
        return mp.mpf(1) / 12
    y = 1 / mp.sqrt(w)
    return (mp.log(y) - 1 / (2 * y) - mp.psi(0, y)) / w


def f_trigamma_asym(w):
    if w == 0:
        return mp.mpf(1) / 6
    y = 1 / mp.sqrt(w)
    return (y * mp.psi(1, y) - 1 - 1 / (2 * y)) / w


def chain(name, pieces):
    """One Horner chain SAM_<NAME>_HORNER(p, w) whose coefficients SAM_<NAME>_SEL picks among the pieces, and the
    centres SAM_<NAME>_C<i> of the pieces fitted in y - c.  pieces: (text, coefficients low..high, centre or None)"""
    deg = max(len(p[1]) for p in pieces) - 1
    lines = ["    /* coefficients by piece (zero above a piece's own degree); one Horner chain of degree %d" % deg]
    lines += ["       %s" % p[0] for p in pieces]
    lines[-1] += " */"
    for k, p in enumerate(pieces):
        if p[2] is not None:
            lines.append("#define SAM_%s_C%d %s" % (name, k, lit(p[2])))

    def sel(j):
        return "SAM_%s_SEL(%s)" % (name, ", ".join(lit(p[1][j]) if j < len(p[1]) else "0.0" for p in pieces))
    lines.append("#define SAM_%s_HORNER(p, w) \\" % name)
    lines.append("    p = %s; \\" % sel(deg))
    for j in range(deg - 1, -1, -1):
        lines.append("    p = fma(p, w, %s);%s" % (sel(j), " \\" if j else ""))
    return lines


def gamma_blocks():
    out = {}
    lines = []
    for name, value in (("GPI", mp.pi), ("GPISQ", mp.pi ** 2), ("HLN2PI", mp.log(2 * mp.pi) / 2), ("PSI_X0", psi_root())):
        hi, lo = hi_lo(value)
        lines += ["#define SAM_%s_HI %s" % (name, hi), "#define SAM_%s_LO %s" % (name, lo)]
    # the largest doubles whose result is below 2^1024, by bisection
    def last_below(f, lo, hi):
        lo, hi = mp.mpf(lo), mp.mpf(hi)
        for _ in range(160):
            mid = (lo + hi) / 2
            lo, hi = (mid, hi) if f(mid) < mp.mpf(2) ** 1024 else (lo, mid)
        v = float(lo)
        return v if mp.mpf(v) <= lo else float(mp.mpf(v) * (1 - mp.mpf(2) ** -53))
    lines.append("#define SAM_TGAMMA_MAX %s" % lit(last_below(mp.gamma, 171, 172)))
    lines.append("#define SAM_LGAMMA_MAX %s" % lit(last_below(mp.loggamma, "2e305", "3e305")))
    out["CONST"] = lines

    def pieces_of(bounds, fs, tag):
        b = [mp.mpf(v) for v in bounds]
        ps = []
        for k, f in enumerate(fs):
            ck, err, cen = fit(f, b[k], b[k + 1], centred=True, nmin=14, nmax=44)
            ps.append(("piece %d: %s, y = c + w, c = %s, y in [%s, %s]: degree %d, error 2^%.1f"
                       % (k, tag[k], lit(cen), lit(b[k]), lit(b[k + 1]), len(ck) - 1, float(mp.log(err, 2))), ck, cen))
        return ps

    def asym(f, b, weight, text):
        hi = 1 / mp.mpf(b) ** 2
        ck, err, _ = fit(f, 0, hi, weight=weight, nmin=5)
        return ("piece 3: %s, w = 1/y^2 in [0, %s]: degree %d, error 2^%.1f (of the function's value)"
                % (text, lit(hi), len(ck) - 1, float(mp.log(err, 2))), ck, None)

    def yw(w):
        return 1 / mp.sqrt(w)
    g = "G = lgamma(y)/((y - 1)(y - 2))"
    ps = pieces_of(LGAMMA_BOUNDS, [f_lgamma] * 3, [g] * 3)
    ps.append(asym(f_stirling, LGAMMA_BOUNDS[3], lambda w: mp.loggamma(yw(w)) * yw(w) if w != 0 else mp.mpf(0),
                   "S = y (lgamma(y) - (y - 1/2) ln y + y - ln(2 pi)/2)"))
    out["LGAMMA"] = chain("LGAMMA", ps)
    ps = pieces_of(DIGAMMA_BOUNDS, [f_digamma0, lambda v: mp.psi(0, v), lambda v: mp.psi(0, v)],
                   ["psi(y)/(y - x0)", "psi(y)", "psi(y)"])
    ps.append(asym(f_digamma_asym, DIGAMMA_BOUNDS[3], lambda w: mp.psi(0, yw(w)) / w if w != 0 else mp.mpf(0),
                   "D = (ln y - 1/(2y) - psi(y))/w"))
    out["DIGAMMA"] = chain("DIGAMMA", ps)
    ps = pieces_of(TRIGAMMA_BOUNDS, [lambda v: mp.psi(1, v)] * 3, ["psi'(y)"] * 3)
    ps.append(asym(f_trigamma_asym, TRIGAMMA_BOUNDS[3], lambda w: yw(w) * mp.psi(1, yw(w)) / w if w != 0 else mp.mpf(0),
                   "T = (y psi'(y) - 1 - 1/(2y))/w"))
    out["TRIGAMMA"] = chain("TRIGAMMA", ps)
    return out


# ---- sa_math_bessel.h ----
#: piece boundaries in x (SAM_<FN>_B<k>): the pieces below 8 are fitted in x - c (I: in x^2), those from 8 on (J, Y, I) and
#: all pieces of K in 1/x - c; below their first boundary Y and K take the logarithmic form
J0_BOUNDS = ("1.5", "4.0", "8.0", "16.0")
J1_BOUNDS = ("1.5", "5.0", "8.0", "16.0")
Y0_BOUNDS = ("0.5", "1.25", "2.5", "5.0", "8.0", "16.0")
Y1_BOUNDS = ("0.5", "1.25", "2.5", "5.0", "8.0", "16.0")
I_BOUNDS = ("8.0", "16.0")
K_BOUNDS = ("1.0", "2.0", "4.0", "8.0", "16.0")


def bessel_zero(f, guess):
    return mp.findroot(f, mp.mpf(guess))


def hankel_pq(n, x):
    chi = x - (mp.mpf(n) / 2 + mp.mpf(1) / 4) * mp.pi
    v = mp.hankel1(n, x) * mp.expj(-chi) * mp.sqrt(mp.pi * x / 2)
    return v.real, v.imag


def bessel_k(n, x):
    """K_n(x) at the working precision.  mpmath's besselk takes seconds per value for an integer order and 16 < x < 150 at
    120 digits; this is the same limit, pi/2 (I_-v - I_v) / sin(pi v) averaged over v = n +- 10^-(dps/2 + 5) (the error
    is of second order in the offset), with the digits the difference cancels added; beyond 200, where Hankel's
    asymptotic series reaches the precision, Tricomi's U."""
    if x > 200:
        return mp.sqrt(mp.pi) * (2 * x) ** n * mp.exp(-x) * mp.hyperu(n + mp.mpf(1) / 2, 2 * n + 1, 2 * x)
    dps = mp.mp.dps
    with mp.workdps(2 * dps + 70 + int(0.9 * float(x))):
        d = mp.mpf(10) ** -(dps // 2 + 5)

        def kv(v):
            return mp.pi / 2 * (mp.besseli(-v, x) - mp.besseli(v, x)) / mp.sin(v * mp.pi)
        r = (kv(n + d) + kv(n - d)) / 2
    return +r


def modulus(n, x):
    return abs(mp.hankel1(n, x))


_JOBS = []


def _run_job(k):
    args, kwargs = _JOBS[k]
    return fit(*args, **kwargs)


def _fit_all():
    """The fits of ``_JOBS`` (independent of each other) over the processors: forked workers read the closures."""
    import multiprocessing
    with multiprocessing.get_context("fork").Pool(min(len(os.sched_getaffinity(0)), 16)) as pool:
        return pool.map(_run_job, range(len(_JOBS)), chunksize=1)


def bessel_blocks():
    """Pass 1 declares every fit (``later``), the fits run in parallel, pass 2 writes the text."""
    del _JOBS[:]
    _bessel_text(None)
    return _bessel_text(_fit_all())


def _bessel_text(results):
    out = {}
    count = [0]

    def fit(*args, **kwargs):                                   # (shadows the module's fit inside this function)
        count[0] += 1
        kwargs.update(npts=200, stride=4)
        if results is None:
            _JOBS.append((args, kwargs))
            return [0.0] * 4, mp.mpf(1), mp.mpf(0)
        return results[count[0] - 1]
    j0z = bessel_zero(lambda v: mp.besselj(0, v), "2.4048")
    j1z = bessel_zero(lambda v: mp.besselj(1, v), "3.8317")
    y0z = bessel_zero(lambda v: mp.bessely(0, v), "0.8936")
    y1z = bessel_zero(lambda v: mp.bessely(1, v), "2.1971")
    lines = []
    for name, value in (("BPIO4", mp.pi / 4), ("BE32", mp.exp(32)), ("J0_Z", j0z), ("J1_Z", j1z), ("Y0_Z", y0z), ("Y1_Z", y1z)):
        hi, lo = hi_lo(value)
        lines += ["#define SAM_%s_HI %s" % (name, hi), "#define SAM_%s_LO %s" % (name, lo)]
    # factors that enter one rounded product or quotient: one word
    for name, value in (("BSQ2OPI", mp.sqrt(2 / mp.pi)), ("B2OPI", 2 / mp.pi), ("BISQ2PI", 1 / mp.sqrt(2 * mp.pi))):
        lines.append("#define SAM_%s %s" % (name, lit(value)))
    out["CONST"] = lines
    tiny = mp.mpf(10) ** -40

    def poly(name, f, hi, text, weight=None):
        """a plain Horner polynomial in z = x^2 on [0, hi] for the small-argument forms"""
        c, err, _ = fit(lambda z: f(mp.sqrt(z if z != 0 else tiny)), 0, hi, weight=weight, nmin=3)
        return (["    /* %s, z = x^2 in [0, %s]: degree %d, error 2^%.1f */" % (text, lit(mp.mpf(hi)), len(c) - 1, float(mp.log(err, 2))),
                 "#define SAM_%s_POLY(p, z) \\" % name, "    p = %s; \\" % lit(c[-1])]
                + ["    p = fma(p, z, %s);%s" % (lit(v), " \\" if k else "") for k, v in reversed(list(enumerate(c[:-1])))])

    def direct(f, bounds, tags, weights, first=0):
        b = [mp.mpf(v) for v in bounds]
        ps = []
        for k, (fk, tag, wk) in enumerate(zip(f, tags, weights)):
            ck, err, cen = fit(fk, b[k], b[k + 1], weight=wk, centred=True, nmin=12, nmax=48)
            ps.append(("piece %d: %s, x = c + w, c = %s, x in [%s, %s]: degree %d, error 2^%.1f"
                       % (k + first, tag, lit(cen), lit(b[k]), lit(b[k + 1]), len(ck) - 1, float(mp.log(err, 2))), ck, cen))
        return ps

    def inverse(f, edges, tag, first, weight=None, limit=None):
        """pieces in t = 1/x - c; edges ascending in x, the last piece reaches t = 0 (``limit``: the value there)"""
        ps = []
        for k in range(len(edges)):
            thi = 1 / mp.mpf(edges[k])
            tlo = 1 / mp.mpf(edges[k + 1]) if k + 1 < len(edges) else mp.mpf(0)
            ck, err, cen = fit(lambda t: limit if t == 0 else f(1 / t), tlo, thi, weight=weight, centred=True, nmin=8, nmax=48)
            ps.append(("piece %d: %s, 1/x = c + w, c = %s, x in [%s, %s]: degree %d, error 2^%.1f"
                       % (k + first, tag, lit(cen), lit(mp.mpf(edges[k])), lit(mp.mpf(edges[k + 1])) if k + 1 < len(edges) else "inf",
                          len(ck) - 1, float(mp.log(err, 2))), ck, cen))
        return ps
    one = (lambda v: mp.mpf(1))
    # ---- J0, J1: direct pieces below 8 (the first zero factored out of its piece), P and Q beyond ----
    for n, fn, zero, bounds in ((0, "J0", j0z, J0_BOUNDS), (1, "J1", j1z, J1_BOUNDS)):
        def jf(v, n=n):
            return mp.besselj(n, v)

        def jzero(v, n=n, zero=zero):
            return mp.diff(lambda u: mp.besselj(n, u), zero) if abs(v - zero) < mp.mpf(10) ** -60 else mp.besselj(n, v) / (v - zero)
        first = jf if n == 0 else (lambda v: mp.mpf(1) / 2 if v == 0 else mp.besselj(1, v) / v)
        ps = direct([first, jzero, jf], ("0.0",) + tuple(bounds[:3]),
                    ["J0(x)" if n == 0 else "J1(x)/x", "J%d(x)/(x - z), z the first zero" % n, "J%d(x), error relative to M%d" % (n, n)],
                    [None, None, lambda v, n=n: modulus(n, v)])
        ps += inverse(lambda v, n=n: hankel_pq(n, v)[0], bounds[2:], "P%d" % n, 3, weight=one, limit=mp.mpf(1))
        out[fn] = chain(fn, ps)
        out[fn + "Q"] = chain(fn + "Q", inverse(lambda v, n=n: hankel_pq(n, v)[1], bounds[2:], "Q%d" % n, 0, weight=one, limit=mp.mpf(0)))
    # ---- Y0, Y1: the logarithmic form below 1/2, direct pieces up to 8, then P and Q of J's chains ----
    c2 = 2 / mp.pi
    out["Y0S"] = (poly("Y0A", lambda v: c2 * mp.besselj(0, v), "0.25", "A = (2/pi) J0(x)")
                  + poly("Y0B", lambda v: mp.bessely(0, v) - c2 * mp.log(v) * mp.besselj(0, v), "0.25", "B = Y0(x) - (2/pi) ln x J0(x)"))
    out["Y1S"] = (poly("Y1A", lambda v: c2 * mp.besselj(1, v) / v, "0.25", "A = (2/pi) J1(x)/x")
                  + poly("Y1B", lambda v: (mp.bessely(1, v) + c2 / v - c2 * mp.log(v) * mp.besselj(1, v)) / v, "0.25",
                         "B = (Y1(x) + (2/pi)/x - (2/pi) ln x J1(x))/x"))
    for n, fn, zero, bounds, zp in ((0, "Y0", y0z, Y0_BOUNDS, 0), (1, "Y1", y1z, Y1_BOUNDS, 1)):
        def yf(v, n=n):
            return mp.bessely(n, v)

        def yzero(v, n=n, zero=zero):
            return mp.diff(lambda u: mp.bessely(n, u), zero) if abs(v - zero) < mp.mpf(10) ** -60 else mp.bessely(n, v) / (v - zero)
        mod = (lambda v, n=n: modulus(n, v))
        fs = [yf] * 4
        ws = [mod] * 4
        tags = ["Y%d(x), error relative to M%d" % (n, n)] * 4
        fs[zp], ws[zp], tags[zp] = yzero, None, "Y%d(x)/(x - z), z the first zero" % n
        if n == 1:
            ws[0], tags[0] = None, "Y1(x)"
        ps = direct(fs, bounds[:5], tags, ws, first=1)
        ps += inverse(lambda v, n=n: hankel_pq(n, v)[0], bounds[4:], "P%d" % n, 5, weight=one, limit=mp.mpf(1))
        out[fn] = chain(fn, ps)
    # ---- I0, I1: the series in z below 8, sqrt(x) exp(-x) I(x) in 1/x beyond ----
    for n in (0, 1):
        fn = "I%d" % n
        small = (lambda v: mp.besseli(0, v)) if n == 0 else (lambda v: mp.besseli(1, v) / v)
        c, err, _ = fit(lambda z, small=small: small(mp.sqrt(z if z != 0 else tiny)), 0, 64, nmin=12, nmax=48)
        ps = [("piece 0: %s, w = x^2 in [0, 64.0]: degree %d, error 2^%.1f"
               % ("I0(x)" if n == 0 else "I1(x)/x", len(c) - 1, float(mp.log(err, 2))), c, None)]
        ps += inverse(lambda v, n=n: mp.sqrt(v) * mp.exp(-v) * mp.besseli(n, v), I_BOUNDS, "sqrt(x) exp(-x) I%d(x)" % n, 1,
                      limit=1 / mp.sqrt(2 * mp.pi))
        out[fn] = chain(fn, ps)
    # ---- K0, K1: the logarithmic form below 1, sqrt(x) exp(x) K(x) in 1/x beyond ----
    out["K0S"] = (poly("K0A", lambda v: mp.besseli(0, v), "1.0", "A = I0(x)")
                  + poly("K0B", lambda v: bessel_k(0, v) + mp.log(v) * mp.besseli(0, v), "1.0", "B = K0(x) + ln x I0(x)"))
    out["K1S"] = (poly("K1A", lambda v: mp.besseli(1, v) / v, "1.0", "A = I1(x)/x")
                  + poly("K1B", lambda v: (bessel_k(1, v) - 1 / v - mp.log(v) * mp.besseli(1, v)) / v, "1.0",
                         "B = (K1(x) - 1/x - ln x I1(x))/x"))
    for n in (0, 1):
        fn = "K%d" % n
        out[fn] = chain(fn, inverse(lambda v, n=n: mp.sqrt(v) * mp.exp(v) * bessel_k(n, v), K_BOUNDS,
                                    "sqrt(x) exp(x) K%d(x)" % n, 1, limit=mp.sqrt(mp.pi / 2)))
    return out


def check(header, text, want):
    with open(header) as fh:
        hdr = fh.read()
    bad = 0
    for macro, value in want.items():               # the boundaries the fits were made for
        m = re.search(r"^#define %s +(\S+)" % macro, hdr, re.M)
        if m is None or float(m.group(1)) != float(value):
            print("%s of %s is not %s" % (macro, header, value))
            bad = 1
    for name, lines in text.items():
        m = re.search(r"/\* BEGIN GENERATED %s\b[^\n]*\n(.*?)\n[^\n]*END GENERATED %s\b" % (name, name), hdr, re.S)
        if m is None or m.group(1).strip() != "\n".join(lines).strip():
            print("block %s of %s differs from the generator's output" % (name, header))
            bad = 1
    return bad


def main():
    which = [w for w in ("inv", "gamma", "bessel") if "--" + w in sys.argv] or ["inv", "gamma", "bessel"]
    bad = 0
    for w in which:
        text = blocks() if w == "inv" else (gamma_blocks() if w == "gamma" else bessel_blocks())
        if "--check" in sys.argv:
            if w == "inv":
                want = {"SAM_ATAN_B%d" % (k + 1): v for k, v in enumerate(ATAN_BOUNDS)}
                want.update({"SAM_ERF_B%d" % (k + 1): v for k, v in enumerate(ERF_BOUNDS)})
                want.update({"SAM_ERFC_B1": ERFC_DIRECT, "SAM_ERFC_CLAMP": ERFC_CLAMP})
                bad |= check(HEADER, text, want)
            elif w == "bessel":
                want = {"SAM_%s_B%d" % (fn, k + 1): v
                        for fn, bs in (("J0", J0_BOUNDS), ("J1", J1_BOUNDS), ("Y0", Y0_BOUNDS), ("Y1", Y1_BOUNDS),
                                       ("I0", I_BOUNDS), ("I1", I_BOUNDS), ("K0", K_BOUNDS), ("K1", K_BOUNDS))
                        for k, v in enumerate(bs)}
                bad |= check(HEADER_BESSEL, text, want)
            else:
                want = {"SAM_%s_B%d" % (fn, k + 1): v for fn, bs in (("LGAMMA", LGAMMA_BOUNDS), ("DIGAMMA", DIGAMMA_BOUNDS),
                                                                      ("TRIGAMMA", TRIGAMMA_BOUNDS)) for k, v in enumerate(bs)}
                bad |= check(HEADER_GAMMA, text, want)
            continue
        for name, lines in text.items():
            print("/* BEGIN GENERATED %s (tools/make_sa_math_coeffs.py) */" % name)
            print("\n".join(lines))
            print("/* END GENERATED %s */" % name)
    if "--check" in sys.argv:
        sys.exit(bad)


if __name__ == "__main__":
    main()
