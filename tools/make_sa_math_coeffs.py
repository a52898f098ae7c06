"""Coefficients of sunode_amd/csrc/sa_math_inv.h (inverse trigonometric / hyperbolic functions, erf, erfc).

Every polynomial of that header is a Chebyshev-node interpolant (near-minimax) computed here with mpmath at 120
digits, converted to the monomial basis of the header's own variable, rounded to double and then MEASURED: the
error of the rounded polynomial against the function, in exact arithmetic, over 1 001 points of the fit
interval.  Nothing is transcribed from another library.

    python tools/make_sa_math_coeffs.py            # prints the literal blocks the header carries
    python tools/make_sa_math_coeffs.py --check    # compares them with the header's text (exit status 1 on a difference)

Sets (variable, interval, form):

  ATAN    P(z) = (t - atan t) / t^3,  z = t^2 in [0, (7/16)^2]          atan t = t - t z P(z)
  ASIN    Q(z) = (asin s - s) / s^3,  z = s^2 in [0, 1/4]               asin s = s + s z Q(z)
  ERF     one Horner chain whose coefficients are selected among the pieces below:
            piece 0   E(z) = erf(s)/s - 1,   z = s^2 in [0, 1]                      erf x = x + x E(x^2)
            piece i   X_i(w) = erfcx(c_i + w),  |w| <= h_i          (argument pieces, a = |x| in [c_i - h_i, c_i + h_i])
            piece j   A_j(w) = a erfcx(a), a = (u_j + w)^(-1/2)     (asymptotic pieces in u = 1/a^2)
          erfcx(a) = exp(a^2) erfc(a).
"""
from __future__ import annotations

import os
import re
import sys

import mpmath as mp

mp.mp.dps = 120
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sunode_amd", "csrc", "sa_math_inv.h")

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
#: error asked of every fit before its coefficients are rounded (relative to the quantity the header forms from it):
#: the rounding of the leading coefficient alone is up to 2^-54, the evaluation's roundings more
TARGET = mp.mpf(2) ** -58


def lit(x) -> str:
    return repr(float(x))


def fit(f, lo, hi, weight=None, target=TARGET, centred=False, nmin=4, nmax=40):
    """Smallest-degree Chebyshev interpolant of f on [lo, hi] (monomial basis in x, or in x - (lo + hi)/2 when
    ``centred``) whose error, BEFORE its coefficients are rounded to double, is below ``target`` relative to
    ``weight(x)`` (default: |f(x)| itself) -- the size of the quantity the header forms from the polynomial.
    -> (double coefficients low..high, that error measured again AFTER the rounding, centre)."""
    lo, hi = mp.mpf(lo), mp.mpf(hi)
    c = (lo + hi) / 2 if centred else mp.mpf(0)
    g = (lambda w: f(c + w))
    a, b = lo - c, hi - c
    pts = [a + (b - a) * mp.mpf(k) / 1000 for k in range(1001)]
    want = [g(w) for w in pts]
    scale = [abs(v) if weight is None else abs(weight(c + w)) for v, w in zip(want, pts)]

    def worst(poly):
        return max(abs(mp.polyval(poly, w) - v) / sc for w, v, sc in zip(pts, want, scale) if sc != 0)
    for n in range(nmin, nmax):
        coeffs = mp.chebyfit(g, [a, b], n)                       # highest power first
        if worst(coeffs) < target:
            rounded = [mp.mpf(float(v)) for v in coeffs]
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


def main():
    text = blocks()
    if "--check" in sys.argv:
        with open(HEADER) as fh:
            hdr = fh.read()
        bad = 0
        want = {"SAM_ATAN_B%d" % (k + 1): v for k, v in enumerate(ATAN_BOUNDS)}
        want.update({"SAM_ERF_B%d" % (k + 1): v for k, v in enumerate(ERF_BOUNDS)})
        want.update({"SAM_ERFC_B1": ERFC_DIRECT, "SAM_ERFC_CLAMP": ERFC_CLAMP})
        for macro, value in want.items():               # the boundaries the fits were made for
            m = re.search(r"^#define %s +(\S+)" % macro, hdr, re.M)
            if m is None or float(m.group(1)) != float(value):
                print("%s of %s is not %s" % (macro, HEADER, value))
                bad = 1
        for name, lines in text.items():
            m = re.search(r"/\* BEGIN GENERATED %s[^\n]*\n(.*?)\n[^\n]*END GENERATED %s" % (name, name), hdr, re.S)
            if m is None or m.group(1).strip() != "\n".join(lines).strip():
                print("block %s of %s differs from the generator's output" % (name, HEADER))
                bad = 1
        sys.exit(bad)
    for name, lines in text.items():
        print("/* BEGIN GENERATED %s (tools/make_sa_math_coeffs.py) */" % name)
        print("\n".join(lines))
        print("/* END GENERATED %s */" % name)


if __name__ == "__main__":
    main()
