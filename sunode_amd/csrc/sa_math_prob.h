/*
 * sa_math_prob.h -- deterministic inverse error functions and incomplete gamma functions:
 * erfinv, erfcinv, gamma(a, x) (lower) and Gamma(a, x) (upper).
 *
 * The fifth block of the math library of the generated callbacks: sunode_amd/symode/codegen.py embeds this text AFTER
 * csrc/sa_math.h, csrc/sa_math_inv.h and csrc/sa_math_gamma.h -- it REQUIRES all three (sa_exp / sa_expm1 / sa_log,
 * sa_erf / sa_erfc, sa_tgamma, sam_log2w, sam_two_sum and the lgamma chain), so they are embedded with it --, and only
 * into the header of a problem whose right-hand side (or one of its derivatives) calls sa_erfinv / sa_erfcinv /
 * sa_igamma_lower / sa_igamma_upper: the headers of all other problems keep their text, and with it their cache keys and
 * code objects.  Same contract as sa_math.h: ONE sequence of IEEE-754 operations (+, -, *, /, sqrt, fabs, explicit
 * fma(), compares and calls of the earlier blocks), compiled by hipcc for gfx950 and by gcc for the oracle with
 * -ffp-contract=off, so the device's values are the host's bit for bit.  No libm / ocml call, no table in memory.
 *
 * erfinv / erfcinv.  Both reduce to one of two cores.  CENTRAL (|p| <= SAM_ERFINV_B1 = 3/4, i.e. erfcinv's argument in
 * [SAM_ERFCINV_B1, SAM_ERFCINV_B2] = [1/4, 7/4]): the Maclaurin series of erfinv through p^9 (0.5 % at 3/4) as the start,
 * polished on f(x) = erf x - p; erfcinv hands p = 1 - y over as TWO words, so nothing of y is lost.  TAIL (q = 1 - |p|
 * or q = y or q = 2 - y below 1/4, each exact): t = sqrt(-2 log(q / 2)) and the classical three-over-four-term
 * rational start (absolute error 4.5e-4 for every q, Abramowitz & Stegun 26.2.23), polished on f(x) = erfc x - q, whose
 * relative accuracy holds down to the smallest normal q -- erfcinv is NEVER erfinv(1 - y).  The polish is
 * SAM_PROB_HALLEY = 2 Halley steps x <- x - u / (1 + x u), u = f / f' (f'' / f' = -2x for both), a FIXED count: the
 * cubic step takes 5e-3 to 1e-7 to below 1e-20, and 3.2e-4 at x = 26.5 to 8e-9 to 1e-22.  erfinv is odd by
 * construction (|x| in, sign copied out).
 *
 * Incomplete gamma functions, 0 < a <= SAM_IGAMMA_AMAX = 32, x >= 0.  One internal pair (sam_igamma_pair): the SMALLER
 * of P(a, x), Q(a, x) is computed directly and the other as the complement.  The pair is kept scaled by Gamma(a) -- it
 * returns P Gamma(a) and Q Gamma(a), the direct one as x^a e^-x times a series or a fraction, the other as
 * sa_tgamma(a) minus it -- because Q alone underflows where Gamma(a, x) is still a normal number (a = 32: a factor
 * 8e33), and because dividing by Gamma(a) only to multiply by it again costs two roundings of sa_tgamma.  Methods:
 *   x <  SAM_IGAMMA_B1 (1/2):   lower series if x^a < 1/2, else the small-a upper series (no cancellation below 0.5615);
 *   x >= SAM_IGAMMA_B1:         lower series if x < a - 1/3 (the median of the distribution), else the continued fraction.
 *   lower series     gamma(a, x) = x^a e^-x / a  sum_n x^n / ((a + 1) ... (a + n))       (positive terms)
 *   fraction         Gamma(a, x) = x^a e^-x / (x + 1 - a - 1 (1 - a) / (x + 3 - a - 2 (2 - a) / (x + 5 - a - ...))),
 *                    evaluated from a level n(a, x) DOWN, not by the forward (modified Lentz) recurrence: see
 *                    sam_igamma_upper_fraction for the measurement behind that
 *   upper series     Gamma(a, x) = ((Gamma(1 + a) - 1) - (x^a - 1)) / a - x^a sum_{n >= 1} (-x)^n / ((a + n) n!)
 *                    with Gamma(1 + a) - 1 = expm1(lgamma(1 + a)) from the lgamma chain in a itself, x^a - 1 = expm1(a log x)
 * The trip counts are run-time and bounded: the series end on a plain compare of the last term with the sum, at
 * SAM_IGAMMA_ITMAX = 512 at the latest; the fraction's depth is [140 / x] + [a] + 8 <= 296, from the arguments alone.
 * The complement Gamma(a) - direct carries sa_tgamma's own error: most of the measured 6.7 ulp, on the line x = a - 1/3.
 *
 * The prefactor x^a e^-x carries its exponent in TWO doubles: log x = h + l (sam_log2w), a h as an exact product,
 * the difference with x by a two-sum; exp of the high word, times 1 + the low word.  (Written as exp(a log x - x) it
 * loses about a |log x| ulps.)
 *
 * Accuracy (tests/test_prob_math.py, against mpmath at 40 digits, on the host build; seeded samples of 200 000 points
 * per function over every piece and both sides of every boundary; the incomplete gamma functions only where the exact
 * result is a normal number, with the lines x = a, x = a - 1/3 and the other method boundaries sampled densely):
 *   erfinv        ceiling 2 ulp, <= 1.82 measured
 *   erfcinv       ceiling 2 ulp, <= 1.83 measured
 *   igamma_lower  ceiling 8 ulp, <= 6.69 measured
 *   igamma_upper  ceiling 8 ulp, <= 5.94 measured
 *
 * Special values: NaN in, NaN out.  erfinv(+-1) = +-inf, NaN beyond, erfinv(+-0) = +-0.  erfcinv(0) = +inf,
 * erfcinv(2) = -inf, NaN outside [0, 2].  Incomplete gamma: x = 0 gives 0 and Gamma(a); x = +inf gives Gamma(a) and 0;
 * a <= 0, a > SAM_IGAMMA_AMAX or x < 0 gives NaN.  A non-finite output makes the callback report a recoverable error,
 * the path the logarithm of a negative state takes.
 */
#ifndef SA_MATH_PROB_H
#define SA_MATH_PROB_H
#define SA_HAVE_MATH_PROB 1

/* The four public functions are real functions on the device, never inlined into a callback (as the Bessel block's):
   one call site of a right-hand side with its derivatives would otherwise carry the error functions, sa_tgamma, both
   series and the fraction several times over -- the code objects of a three-state model took more than ten minutes
   each to compile that way.  The helpers stay SA_FN.  The operation sequence, and with it every bit of the result, is
   the same either way. */
#ifdef __HIP__
#define SAM_PROB_FN static __device__ __attribute__((noinline))
#else
#define SAM_PROB_FN SA_FN
#endif

#define SAM_PROB_HALLEY 2                /* polish steps of the inverse error functions (a fixed count) */
#define SAM_2_OVER_SQRTPI 1.1283791670955126

/* ---- erfinv / erfcinv ---- */
#define SAM_ERFINV_B1 0.75               /* |x| above: the tail core in q = 1 - |x| */
#define SAM_ERFCINV_B1 0.25              /* x below: the tail core in q = x */
#define SAM_ERFCINV_B2 1.75              /* x above: the tail core in q = 2 - x, negated */

/* erfinv(ph + pl), 0 <= ph <= 3/4, |pl| <= ulp(ph)/2 */
SA_FN double sam_erfinv_central(double ph, double pl)
{
    const double z = ph * ph;
    /* sqrt(pi)/2 (1 + pi/12 z + 7 pi^2/480 z^2 + 127 pi^3/40320 z^3 + 4369 pi^4/5806080 z^4) */
    double s = 0.07329907936638086;
    s = fma(s, z, 0.09766361950392055);
    s = fma(s, z, 0.1439313791725826);
    s = fma(s, z, 0.2617993877991494);
    s = fma(s, z, 1.0);
    double x = ph * (0.886226925452758 * s);
    for (int k = 0; k < SAM_PROB_HALLEY; k++) {
        const double f = (sa_erf(x) - ph) - pl;
        const double u = f / (SAM_2_OVER_SQRTPI * sa_exp(-(x * x)));
        x = x - u / fma(x, u, 1.0);
    }
    return x;
}

/* the x > 0 with erfc x = q, 0 < q < 1/4 */
SA_FN double sam_erfcinv_tail(double q)
{
    const double t = sqrt(-2.0 * (sa_log(q) - SAM_LN2));
    const double num = fma(fma(0.010328, t, 0.802853), t, 2.515517);
    const double den = fma(fma(fma(0.001308, t, 0.189269), t, 1.432788), t, 1.0);
    double x = 0.7071067811865476 * (t - num / den);
    for (int k = 0; k < SAM_PROB_HALLEY; k++) {
        const double f = sa_erfc(x) - q;
        const double u = f / (-SAM_2_OVER_SQRTPI * sa_exp(-(x * x)));
        x = x - u / fma(x, u, 1.0);
    }
    return x;
}

SAM_PROB_FN double sa_erfinv(double x)
{
    const double a = fabs(x);
    if (!(a < 1.0)) return (a == 1.0) ? sam_copysign(SAM_INF, x) : SAM_NAN;
    const double r = (a <= SAM_ERFINV_B1) ? sam_erfinv_central(a, 0.0) : sam_erfcinv_tail(1.0 - a);
    return sam_copysign(r, x);
}

SAM_PROB_FN double sa_erfcinv(double x)
{
    if (!(x > 0.0 && x < 2.0)) return (x == 0.0) ? SAM_INF : ((x == 2.0) ? -SAM_INF : SAM_NAN);
    if (x < SAM_ERFCINV_B1) return sam_erfcinv_tail(x);
    if (x > SAM_ERFCINV_B2) return -sam_erfcinv_tail(2.0 - x);
    double p;
    const double pl = sam_two_sum(1.0, -x, &p);                  /* 1 - x = p + pl exactly */
    const int neg = p < 0.0;
    const double r = sam_erfinv_central(neg ? -p : p, neg ? -pl : pl);
    return neg ? -r : r;
}

/* ---- incomplete gamma functions ---- */
#define SAM_IGAMMA_AMAX 32.0
#define SAM_IGAMMA_B1 0.5                /* x below: the direct upper function is the alternating series, from here on the fraction */
#define SAM_IGAMMA_ITMAX 512             /* bound of the series' trip counts (the domain takes 90) */
#define SAM_IGAMMA_EPS 5.551115123125783e-17     /* 2^-54: a term below it times the sum ends a series */
#define SAM_IGAMMA_FRAC_NX 140.0         /* the fraction is evaluated from level [140 / x] + [a] + 8 down: at most 296 */
#define SAM_IGAMMA_MLN2 -0.6931471805599453

/* x^a e^-x for 0 < a <= AMAX and a finite x > 0: the exponent a log x - x in two words */
SA_FN double sam_igamma_prefactor(double a, double x)
{
    double h, l, s;
    sam_log2w(x, &h, &l);
    const double th = a * h;
    const double tl = fma(a, h, -th) + a * l;
    const double e = sam_two_sum(th, -x, &s);
    const double r = sa_exp(s);
    return fma(r, e + tl, r);
}

/* gamma(a, x) by the lower series; the sum carries its rounding errors along (sam_two_sum) */
SA_FN double sam_igamma_lower_series(double a, double x)
{
    double ap = a, term = 1.0, sum = 1.0, err = 0.0;
    for (int n = 0; n < SAM_IGAMMA_ITMAX; n++) {
        ap = ap + 1.0;
        term = term * (x / ap);
        err = err + sam_two_sum(sum, term, &sum);
        if (term <= sum * SAM_IGAMMA_EPS) break;
    }
    return sam_igamma_prefactor(a, x) * (sum + err) / a;
}

/* Gamma(a, x) by the continued fraction, x >= 1/2 and x >= a - 1/3: f_k = b_k + a_(k+1) / f_(k+1) with
   b_k = x + 2k + 1 - a, a_k = -k (k - a), evaluated from the level n down to 0, Gamma(a, x) = x^a e^-x / f_0.  Every f_k is
   positive here (the numerators are positive up to k = a; beyond, f_(k+1) > k), and a level damps the error of the
   levels below it, so the result carries the roundings of the last levels only -- the forward (modified Lentz) form
   multiplies n ratios together and was measured 52 ulp off at x = 1.1, where it needs 83 of them.  n is a function of
   the arguments alone: the truncation error falls like exp(-4 sqrt(n x)) once k has passed a (measured: n x = 113 at
   x = 1/2, 120 at 3/2, 170 at 10, 280 at 40, n = 3 at x = 700 suffice for 2^-58), so n = [140 / x] + [a] + 8. */
SA_FN double sam_igamma_upper_fraction(double a, double x)
{
    const int n = (int)(SAM_IGAMMA_FRAC_NX / x) + (int)a + 8;
    const double xa = x - a;
    double f = xa + (2.0 * (double)n + 1.0);
    for (int k = n; k >= 1; k--) {
        const double dk = (double)k;
        f = (xa + (2.0 * dk - 1.0)) - dk * (dk - a) / f;
    }
    return sam_igamma_prefactor(a, x) / f;
}

/* Gamma(a, x) for 0 < x < 1/2 and x^a >= 1/2 (so a < 1): the alternating series, with Gamma(1 + a) - 1 and x^a - 1
   formed without cancellation.  Below exp(-gamma_E) = 0.5615 both terms of the result are positive for every a. */
SA_FN double sam_igamma_upper_series(double a, double x)
{
    /* lgamma(1 + a) = a (a - 1) G(1 + a): the pieces [3/4, 3/2] and [3/2, 3] of the lgamma chain, centred in a */
    const int k1 = a >= 0.5, k2 = 0, k3 = 0;
    const double w = a - (k1 ? SAM_LGAMMA_C1 - 1.0 : SAM_LGAMMA_C0 - 1.0);
    double p;
    SAM_LGAMMA_HORNER(p, w);
    const double g1 = sa_expm1((a * (a - 1.0)) * p);             /* Gamma(1 + a) - 1 */
    const double pm1 = sa_expm1(a * sa_log(x));                  /* x^a - 1 */
    double t = 1.0, sum = 0.0, err = 0.0;
    for (int n = 1; n <= SAM_IGAMMA_ITMAX; n++) {
        const double dn = (double)n;
        t = t * (-x / dn);
        const double v = t / (a + dn);
        err = err + sam_two_sum(sum, v, &sum);
        if (fabs(v) <= fabs(sum) * SAM_IGAMMA_EPS) break;
    }
    return (g1 - pm1) / a - (pm1 + 1.0) * (sum + err);
}

/* lo = gamma(a, x) = P Gamma(a), up = Gamma(a, x) = Q Gamma(a); 0 < a <= AMAX, x > 0 finite.  The lower function is the
   direct one where it is the smaller: below the median of the distribution, taken as x^a < 1/2 for x < 1/2 (P is
   x^a / Gamma(1 + a) times a factor in (0.8, 1) there) and as x < a - 1/3 from there on. */
SA_FN void sam_igamma_pair(double a, double x, double *lo_out, double *up_out)
{
    const double g = sa_tgamma(a);
    const int tiny = x < SAM_IGAMMA_B1;
    const int lower = tiny ? (a * sa_log(x) < SAM_IGAMMA_MLN2) : (x < a - 1.0 / 3.0);
    if (lower) {
        const double v = sam_igamma_lower_series(a, x);
        *lo_out = v;
        *up_out = g - v;
    } else {
        const double v = tiny ? sam_igamma_upper_series(a, x) : sam_igamma_upper_fraction(a, x);
        *up_out = v;
        *lo_out = g - v;
    }
}

/* 0: the ordinary case; otherwise lo / up hold the special values */
SA_FN int sam_igamma_special(double a, double x, double *lo_out, double *up_out)
{
    if (!(a > 0.0 && a <= SAM_IGAMMA_AMAX && x >= 0.0)) { *lo_out = SAM_NAN; *up_out = SAM_NAN; return 1; }
    if (x == 0.0) { *lo_out = 0.0; *up_out = sa_tgamma(a); return 1; }
    if (x == SAM_INF) { *lo_out = sa_tgamma(a); *up_out = 0.0; return 1; }
    return 0;
}

SAM_PROB_FN double sa_igamma_lower(double a, double x)
{
    double lo, up;
    if (!sam_igamma_special(a, x, &lo, &up)) sam_igamma_pair(a, x, &lo, &up);
    return lo;
}

SAM_PROB_FN double sa_igamma_upper(double a, double x)
{
    double lo, up;
    if (!sam_igamma_special(a, x, &lo, &up)) sam_igamma_pair(a, x, &lo, &up);
    return up;
}
#endif /* SA_MATH_PROB_H */
