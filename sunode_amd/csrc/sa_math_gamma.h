/*
 * sa_math_gamma.h -- deterministic gamma-family functions: log|Gamma|, Gamma, digamma (psi), trigamma (psi').
 *
 * The third block of the math library of the generated callbacks: sunode_amd/symode/codegen.py embeds this text AFTER
 * csrc/sa_math.h (and after csrc/sa_math_inv.h where that is present), and only into the header of a problem whose
 * right-hand side (or one of its derivatives) calls sa_lgamma / sa_tgamma / sa_digamma / sa_trigamma -- the headers of
 * all other problems keep their text, and with it their cache keys and code objects.  Same contract as sa_math.h: ONE
 * sequence of IEEE-754 operations (+, -, *, /, fabs, floor, explicit fma(), integer bit operations, and sa_exp / sa_log
 * and the kernels sam_split / sam_log_poly / sam_sin_k / sam_cos_k of the first block), compiled by hipcc for gfx950 and
 * by gcc for the oracle with -ffp-contract=off, so the device's values are the host's bit for bit.  No libm / ocml call,
 * no table in memory.
 *
 * Intervals without divergence: every function maps its argument to y >= 3/4 (x itself; x + 1 for a small x; 1 - x or
 * -x for a negative x, kept as two words where the sum rounds), selects the coefficients and the centre of y's piece
 * with ternaries (v_cndmask on the device) and runs ONE Horner chain; the pieces of large y are the asymptotic series
 * in 1/y^2.  The upward recurrence of sa_tgamma (Gamma(x) = Gamma(x + n) / (x (x + 1) ... (x + n - 1)), x + n in
 * [6, 7)) has SIX stages whose factors are switched to 1 by selects.  Only the special-value exits and the reflection
 * of a negative argument branch.  The piece boundaries are the SAM_<FN>_B<k> definitions below
 * (codegen.math_gamma_boundaries() reads them for the tests).
 *
 * Zeros keep their relative accuracy: lgamma is formed as (y - 1)(y - 2) G(y) around 1 and 2, digamma as
 * (y - x0) P(y) around its positive root x0 = 1.4616..., x0 in two words.  sa_tgamma forms
 * exp((y - 1/2) ln y - y + ...) with the exponent in two words, from a two-word logarithm (sam_log2w: the h + l
 * logarithm of sa_pow, restated here because sa_math.h stays as it is), and divides by the two-word product of the
 * recurrence.  Negative arguments go through the reflection formulas; sin(pi x), cos(pi x) come from an exact
 * reduction of x modulo 1 to [0, 1/4] (sam_sincospi), never from sa_sin(pi * x).
 *
 * Coefficients: tools/make_sa_math_coeffs.py (Chebyshev-node fits with mpmath at 120 digits; the fit interval and
 * the measured error of the rounded polynomial stand beside every set).  `--check` compares this file with its output.
 *
 * Accuracy (tests/test_gamma_math.py, against mpmath at 200 bits; worst case over the test's seeded sample of 1 500
 * points per range -- a larger sample finds more, e.g. 2.9 ulp for tgamma near 169 --, ceiling 4 ulp; for lgamma /
 * digamma at x < 0, where the reflection cancels, in units of spacing(max(|f(x)|, |f(1 - x)|))):
 *   lgamma    1.16 over 1e-300 .. 1e300, 1.63 on (0, 30), 2.26 / 1.79 within 0.1 of the zeros 1 / 2, 1.75 on (-12, 0)
 *   tgamma    1.62 on (0, 171.6), 1.24 over 1e-300 .. 1, 2.07 on (-170, 0)  (scipy.special.gamma: 4.74, <= 4, 9.17);
 *             subnormal results on (-184, -170.6): within 4 steps of 2^-1074
 *   digamma   1.06 over 1e-300 .. 1e300, 1.76 on (0, 30), 2.02 within 0.1 of the root x0, 2.32 on (-12, 0)
 *   trigamma  1.86 over 1e-150 .. 1e300, 1.54 on (0, 30), 2.29 on (-12, 0)
 * (negative ranges: at least 1e-3 away from the poles and, lgamma / digamma, from the zeros).
 *
 * Special values: NaN in, NaN out.  Poles 0, -1, -2, ...: lgamma +inf, tgamma(+-0) = +-inf and NaN at the negative
 * integers (C99 F.10.8.4), digamma NaN, trigamma +inf.  +inf: lgamma, tgamma, digamma +inf, trigamma +0.  -inf: lgamma
 * +inf, the others NaN.  lgamma(1) = lgamma(2) = +0.  tgamma overflows to +inf above SAM_TGAMMA_MAX (171.62...) and
 * underflows to +-0, with the sign of Gamma, for large negative non-integers.  A non-finite output makes the callback
 * report a recoverable error, the path the logarithm of a negative state takes.
 */
#ifndef SA_MATH_GAMMA_H
#define SA_MATH_GAMMA_H
#define SA_HAVE_MATH_GAMMA 1

/* BEGIN GENERATED CONST (tools/make_sa_math_coeffs.py) */
#define SAM_GPI_HI 3.141592653589793
#define SAM_GPI_LO 1.2246467991473532e-16
#define SAM_GPISQ_HI 9.869604401089358
#define SAM_GPISQ_LO 6.265295508739711e-16
#define SAM_HLN2PI_HI 0.9189385332046728
#define SAM_HLN2PI_LO -3.8782941580672414e-17
#define SAM_PSI_X0_HI 1.4616321449683622
#define SAM_PSI_X0_LO 9.549995429965697e-17
#define SAM_TGAMMA_MAX 171.6243769563027
#define SAM_LGAMMA_MAX 2.5599833278516383e+305
/* END GENERATED CONST */

/* log x = h + l for a finite x > 0, to about 2^-59 of |log m| + 2^-105 of |e ln 2| (x = m 2^e): the quotient
   s = f / (2 + f) as a double-double, the odd series in s, e ln 2 in two words (the logarithm inside sa_pow) */
SA_FN void sam_log2w(double x, double *h_out, double *l_out)
{
    int e;
    const double f = sam_split(x, &e) - 1.0;
    const double d = 2.0 + f;
    const double dl = f - (d - 2.0);
    const double sh = f / d;
    const double sl = fma(-sh, dl, fma(-sh, d, f)) / d;
    const double T = 0.5 * sam_log_poly(sh * sh);                /* log(m) = 2 s (1 + T) */
    const double dk = (double)e;
    const double A = dk * SAM_LN2_HI, Bq = 2.0 * sh;
    const double h0 = A + Bq;
    const double bb = h0 - A;
    const double er = (A - (h0 - bb)) + (Bq - bb);               /* two-sum */
    const double l0 = er + fma(dk, SAM_LN2_LO, fma(Bq, T, 2.0 * sl));
    const double h = h0 + l0;
    *h_out = h;
    *l_out = (h0 - h) + l0;
}

/* a + b = s + (returned error), exactly */
SA_FN double sam_two_sum(double a, double b, double *s_out)
{
    const double s = a + b;
    const double bb = s - a;
    *s_out = s;
    return (a - (s - bb)) + (b - bb);
}

/* sin(pi x) and cos(pi x), |x| < 2^52: n = the integer nearest to x, f = x - n exactly (|f| <= 1/2), |f| folded to
   r in [0, 1/4] exactly, pi r in two words */
SA_FN void sam_sincospi(double x, double *s_out, double *c_out)
{
    const double n = floor(x + 0.5);
    const double f = x - n;
    const double hn = 0.5 * n;
    const int odd = floor(hn) != hn;
    const double a = fabs(f);
    const int sw = a > 0.25;
    const double r = sw ? 0.5 - a : a;
    const double ph = r * SAM_GPI_HI;
    const double pl = fma(r, SAM_GPI_HI, -ph) + r * SAM_GPI_LO;
    const double s = sam_sin_k(ph, pl), c = sam_cos_k(ph, pl);
    const double sv = sw ? c : s, cv = sw ? s : c;               /* sin(pi |f|), cos(pi |f|) */
    *s_out = (odd != (f < 0.0)) ? -sv : sv;
    *c_out = odd ? -cv : cv;
}

/* ---- lgamma ---- */
#define SAM_LGAMMA_B1 0.75       /* below: lgamma x = lgamma(x + 1) - ln x */
#define SAM_LGAMMA_B2 1.5
#define SAM_LGAMMA_B3 3.0
#define SAM_LGAMMA_B4 6.0        /* from here on: Stirling's series */
#define SAM_LGAMMA_B5 1e17       /* from here on lgamma x = x (ln x - 1) to 2^-55 */
/* (the SEL macros read the piece flags k1, k2, k3 of the ENCLOSING scope: every user of a HORNER macro declares them;
   sam_gamma_core sets all three to use the last piece alone) */
#define SAM_LGAMMA_SEL(c0, c1, c2, c3) (k2 ? (k3 ? (c3) : (c2)) : (k1 ? (c1) : (c0)))
/* BEGIN GENERATED LGAMMA (tools/make_sa_math_coeffs.py) */
    /* coefficients by piece (zero above a piece's own degree); one Horner chain of degree 21
       piece 0: G = lgamma(y)/((y - 1)(y - 2)), y = c + w, c = 1.125, y in [0.75, 1.5]: degree 21, error 2^-55.4
       piece 1: G = lgamma(y)/((y - 1)(y - 2)), y = c + w, c = 2.25, y in [1.5, 3.0]: degree 21, error 2^-55.3
       piece 2: G = lgamma(y)/((y - 1)(y - 2)), y = c + w, c = 4.5, y in [3.0, 6.0]: degree 21, error 2^-54.6
       piece 3: S = y (lgamma(y) - (y - 1/2) ln y + y - ln(2 pi)/2), w = 1/y^2 in [0, 0.027777777777777776]: degree 6, error 2^-59.9 (of the function's value) */
#define SAM_LGAMMA_C0 1.125
#define SAM_LGAMMA_C1 2.25
#define SAM_LGAMMA_C2 4.5
#define SAM_LGAMMA_HORNER(p, w) \
    p = SAM_LGAMMA_SEL(-0.0033364909969457747, -1.4922144283217354e-09, -6.404641163013001e-16, 0.0); \
    p = fma(p, w, SAM_LGAMMA_SEL(0.003918081961976261, 3.4958112706149023e-09, 2.9922582450264672e-15, 0.0)); \
    p = fma(p, w, SAM_LGAMMA_SEL(-0.0020294170904300458, -3.5873906270594855e-09, -6.0774796097749786e-15, 0.0)); \
    p = fma(p, w, SAM_LGAMMA_SEL(0.0024052181994097407, 8.474513322443875e-09, 2.8624402107412467e-14, 0.0)); \
    p = fma(p, w, SAM_LGAMMA_SEL(-0.0037204410759091927, -2.6237256986129076e-08, -1.7751053949185725e-13, 0.0)); \
    p = fma(p, w, SAM_LGAMMA_SEL(0.004420031627777158, 6.211268218830923e-08, 8.378631810677121e-13, 0.0)); \
    p = fma(p, w, SAM_LGAMMA_SEL(-0.005105140931733737, -1.4280824653864626e-07, -3.838307468754579e-12, 0.0)); \
    p = fma(p, w, SAM_LGAMMA_SEL(0.006109528539288366, 3.403303586159362e-07, 1.823926873003976e-11, 0.0)); \
    p = fma(p, w, SAM_LGAMMA_SEL(-0.007360499725206367, -8.162885225940421e-07, -8.724549344562815e-11, 0.0)); \
    p = fma(p, w, SAM_LGAMMA_SEL(0.008885442652873304, 1.9610309298135665e-06, 4.180204671814476e-10, 0.0)); \
    p = fma(p, w, SAM_LGAMMA_SEL(-0.010782953470194624, -4.734544076564375e-06, -2.013120642786258e-09, 0.0)); \
    p = fma(p, w, SAM_LGAMMA_SEL(0.013170624359593543, 1.1501953265681634e-05, 9.756994798244571e-09, 0.0)); \
    p = fma(p, w, SAM_LGAMMA_SEL(-0.016209048129205757, -2.8149289639083216e-05, -4.7646164310769474e-08, 0.0)); \
    p = fma(p, w, SAM_LGAMMA_SEL(0.020132841860418065, 6.952279516229163e-05, 2.3481743479848546e-07, 0.0)); \
    p = fma(p, w, SAM_LGAMMA_SEL(-0.025296547269316964, -0.00017370931765654704, -1.170602460720543e-06, 0.0)); \
    p = fma(p, w, SAM_LGAMMA_SEL(0.03226388713791912, 0.0004406567320300957, 5.9215542411674835e-06, 0.004298394281325464)); \
    p = fma(p, w, SAM_LGAMMA_SEL(-0.041994856012586367, -0.001140986590005892, -3.0534844137413286e-05, -0.0018449995052567591)); \
    p = fma(p, w, SAM_LGAMMA_SEL(0.05628216876911452, 0.0030411186579069323, 0.00016163193136506986, 0.0008404447851602169)); \
    p = fma(p, w, SAM_LGAMMA_SEL(-0.07892681966460653, -0.00846402499357528, -0.0008884513143032816, -0.0005952257418022643)); \
    p = fma(p, w, SAM_LGAMMA_SEL(0.11960320844256032, 0.025268354959288596, 0.005179866342315459, 0.0007936507373369848)); \
    p = fma(p, w, SAM_LGAMMA_SEL(-0.21115323425817586, -0.08588084755126099, -0.03356471927391053, -0.0027777777776807643)); \
    p = fma(p, w, SAM_LGAMMA_SEL(0.5487833977237905, 0.3995894876556691, 0.2804270366677077, 0.0833333333333333));
/* END GENERATED LGAMMA */
/* x > 0 finite, x <= SAM_LGAMMA_MAX */
SA_FN double sam_lgamma_pos(double x)
{
    const int small = x < SAM_LGAMMA_B1;
    const double y = small ? x + 1.0 : x;
    const int k1 = y >= SAM_LGAMMA_B2, k2 = y >= SAM_LGAMMA_B3, k3 = y >= SAM_LGAMMA_B4;
    const double iy = 1.0 / y;
    const double cen = (k2 ? SAM_LGAMMA_C2 : (k1 ? SAM_LGAMMA_C1 : SAM_LGAMMA_C0)) - (small ? 1.0 : 0.0);
    const double w = k3 ? iy * iy : x - cen;
    double p;
    SAM_LGAMMA_HORNER(p, w);
    const double u1 = small ? x : x - 1.0, u2 = small ? x - 1.0 : x - 2.0;       /* y - 1 and y - 2, exactly */
    const double mid = (u1 * u2) * p + 0.0;                                     /* (+ 0.0: lgamma 1 = +0) */
    double h, l;
    sam_log2w(x, &h, &l);
    /* Stirling: (x - 1/2) ln x - x + ln(2 pi)/2 + S(1/x^2)/x, the product in two words */
    const double a = x - 0.5;
    const double th = a * h;
    const double tl = fma(a, h, -th) + a * l;
    double s;
    const double e = sam_two_sum(th, -x, &s);
    const double stir = s + (SAM_HLN2PI_HI + (p * iy + ((e + tl) + SAM_HLN2PI_LO)));
    const double hm = h - 1.0;
    const double huge = x * (hm + (((h - hm) - 1.0) + l));
    return k3 ? ((x >= SAM_LGAMMA_B5) ? huge : stir) : (small ? (mid - h) - l : mid);
}

SA_FN double sa_lgamma(double x)
{
    if (!(x == x)) return x;
    const double ax = fabs(x);
    if (ax == SAM_INF || ax == 0.0) return SAM_INF;
    if (x > 0.0) return (x > SAM_LGAMMA_MAX) ? SAM_INF : sam_lgamma_pos(x);
    if (floor(x) == x) return SAM_INF;                           /* the poles -1, -2, ... */
    if (ax < 1.3877787807814457e-17) return -sa_log(ax);          /* 2^-56: Gamma(x) = 1/x - gamma_E + ... */
    /* |Gamma(x)| = pi / (|x sin(pi x)| Gamma(-x)): the logarithm of the quotient in two words */
    double sn, cs, h, l;
    sam_sincospi(x, &sn, &cs);
    sn = fabs(sn);
    const double dh = ax * sn, dl = fma(ax, sn, -dh);
    const double q = SAM_GPI_HI / dh;
    const double ql = (fma(-q, dh, SAM_GPI_HI) + (SAM_GPI_LO - q * dl)) / dh;
    sam_log2w(q, &h, &l);
    return (h - sam_lgamma_pos(ax)) + (l + ql / q);
}

/* ---- tgamma ---- */
#define SAM_TGAMMA_B1 6.0        /* below: the upward recurrence lifts x into [6, 7); SAM_TGAMMA_STAGES factors */
#define SAM_TGAMMA_STAGES 6
/* x > 0 finite: Gamma(x) = exp(E) / P, E = eh + el, P = ph + pl */
SA_FN void sam_gamma_core(double x, double *eh_out, double *el_out, double *ph_out, double *pl_out)
{
    double yh = x, yl = 0.0, ph = 1.0, pl = 0.0;
    for (int k = 0; k < SAM_TGAMMA_STAGES; k++) {                /* (a compile-time trip count) */
        const int act = yh < SAM_TGAMMA_B1;
        const double fh = act ? yh : 1.0, fl = act ? yl : 0.0, inc = act ? 1.0 : 0.0;
        const double nh = ph * fh;
        pl = fma(ph, fh, -nh) + fma(ph, fl, pl * fh);
        ph = nh;
        double s;
        yl = yl + sam_two_sum(yh, inc, &s);
        yh = s;
    }
    const int k1 = 1, k2 = 1, k3 = 1;                            /* the Stirling piece of the lgamma chain */
    const double iy = 1.0 / yh;
    const double w = iy * iy;
    double p, h, l, s, E0;
    SAM_LGAMMA_HORNER(p, w);
    sam_log2w(yh, &h, &l);
    const double a = yh - 0.5;
    const double th = a * h;
    const double tl = fma(a, h, -th) + a * l;
    const double e = sam_two_sum(th, -yh, &s);
    /* yl enters through d/dy of the exponent, ln y - 1/(2y) */
    const double low = (p * iy + SAM_HLN2PI_LO) + ((e + tl) + yl * (h - 0.5 * iy));
    const double e2 = sam_two_sum(s, SAM_HLN2PI_HI, &E0) + low;
    const double eh = E0 + e2;
    *eh_out = eh;
    *el_out = (E0 - eh) + e2;
    *ph_out = ph;
    *pl_out = pl;
}

SA_FN double sa_tgamma(double x)
{
    if (!(x == x)) return x;
    const double ax = fabs(x);
    if (ax < 1.3877787807814457e-17) return 1.0 / x;             /* 2^-56; +-0 -> +-inf */
    if (x == SAM_INF || x > SAM_TGAMMA_MAX) return SAM_INF;
    if (x < 0.0 && (ax == SAM_INF || floor(x) == x)) return SAM_NAN;
    double eh, el, ph, pl;
    sam_gamma_core(ax, &eh, &el, &ph, &pl);
    if (x > 0.0) {
        const double r = sa_exp(eh) / ph;
        return (r == SAM_INF) ? r : fma(r, el - pl / ph, r);
    }
    /* Gamma(x) = pi P exp(-E) / (|x| sin(pi x)); beyond E = 650 the exponent is shifted by 128 ln 2 and the result
       scaled by 2^-128 at the end, so that a subnormal result is rounded once */
    double sn, cs, t;
    sam_sincospi(x, &sn, &cs);
    const int far = eh > 650.0;
    const double sh = far ? 88.722839111673 : 0.0, slo = far ? 2.9683799217232634e-15 : 0.0;          /* 128 ln 2 = sh + slo */
    const double te = sam_two_sum(eh, -sh, &t);
    const double dh = ax * sn, dl = fma(ax, sn, -dh);
    const double nh = SAM_GPI_HI * ph, nl = fma(SAM_GPI_HI, ph, -nh) + fma(SAM_GPI_LO, ph, SAM_GPI_HI * pl);
    const double q = nh / dh;
    const double ql = (fma(-q, dh, nh) + (nl - q * dl)) / dh;   /* pi P / (|x| sin(pi x)) = q + ql */
    const double r = q * sa_exp(-t);
    const double v = fma(r, ql / q - ((te + el) - slo), r);
    /* an underflow of exp(-t) leaves r = +-0 with the sign of Gamma: the correction must not touch it ((+0) + (-0) = +0) */
    return (r == 0.0) ? r : (far ? v * 2.938735877055719e-39 : v);               /* 2^-128 */
}

/* ---- digamma ---- */
#define SAM_DIGAMMA_B1 1.0       /* below: psi x = psi(x + 1) - 1/x */
#define SAM_DIGAMMA_B2 2.0
#define SAM_DIGAMMA_B3 4.0
#define SAM_DIGAMMA_B4 8.0       /* from here on: ln y - 1/(2y) - D(1/y^2)/y^2 */
#define SAM_DIGAMMA_SEL(c0, c1, c2, c3) (k2 ? (k3 ? (c3) : (c2)) : (k1 ? (c1) : (c0)))
/* BEGIN GENERATED DIGAMMA (tools/make_sa_math_coeffs.py) */
    /* coefficients by piece (zero above a piece's own degree); one Horner chain of degree 23
       piece 0: psi(y)/(y - x0), y = c + w, c = 1.5, y in [1.0, 2.0]: degree 22, error 2^-54.2
       piece 1: psi(y), y = c + w, c = 3.0, y in [2.0, 4.0]: degree 23, error 2^-54.0
       piece 2: psi(y), y = c + w, c = 6.0, y in [4.0, 8.0]: degree 22, error 2^-54.8
       piece 3: D = (ln y - 1/(2y) - psi(y))/w, w = 1/y^2 in [0, 0.015625]: degree 5, error 2^-58.1 (of the function's value) */
#define SAM_DIGAMMA_C0 1.5
#define SAM_DIGAMMA_C1 3.0
#define SAM_DIGAMMA_C2 6.0
#define SAM_DIGAMMA_HORNER(p, w) \
    p = SAM_DIGAMMA_SEL(0.0, 7.108977174651833e-12, 0.0, 0.0); \
    p = fma(p, w, SAM_DIGAMMA_SEL(0.00011881232908510335, -2.1332191571834103e-11, -2.5297724320396582e-18, 0.0)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(-0.0001782188548855923, 2.1363796247022648e-11, 1.5243352337420053e-17, 0.0)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(9.653646261410062e-05, -6.4144390367226e-11, -3.373435776456977e-17, 0.0)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(-0.00014480643368061614, 3.046124298704505e-10, 2.0417990782850773e-16, 0.0)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(0.00032395945401345196, -9.147759692625141e-10, -1.8196118097640648e-15, 0.0)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(-0.00048595039220036254, 2.579267241968924e-09, 1.1023583469196389e-14, 0.0)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(0.0006909255761282986, -7.752903093043211e-09, -6.358645225478366e-14, 0.0)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(-0.0010364584817312839, 2.3481158346701657e-08, 3.8693346593790523e-13, 0.0)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(0.0015633696313653504, -7.069062318489005e-08, -2.3728023701308194e-12, 0.0)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(-0.0023454947397380833, 2.1297418115106333e-07, 1.4524687818949358e-11, 0.0)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(0.003518106563802472, -6.430211938810789e-07, -8.924177143602937e-11, 0.0)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(-0.005279937255532708, 1.945929605753433e-06, 5.512332674209807e-10, 0.0)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(0.007927021796868154, -5.907358013123235e-06, -3.4262720152645286e-09, 0.0)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(-0.011908220105959716, 1.801262758814673e-05, 2.1465700043993997e-08, 0.0)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(0.017907248317313294, -5.5267825392302674e-05, -1.3586539061614036e-07, 0.0)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(-0.026975796659787055, 0.0001711061979683179, 8.716186018596205e-07, 0.0)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(0.040760833940846085, -0.0005367773819947723, -5.6948548454377025e-06, 0.0)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(-0.06192213327548831, 0.0017180619844478504, 3.817924696766235e-05, -0.017711160415846534)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(0.09498872445289039, -0.005677755143366058, -0.00026596630592133137, 0.007519088230747095)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(-0.14840492305388092, 0.019823233711138217, 0.0019713046987923, -0.004166217650696842)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(0.24054248424078697, -0.07705690315959436, -0.01639486612255725, 0.003968252342841619)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(-0.4236274212814606, 0.39493406684822646, 0.18132295573711535, -0.008333333331168558)); \
    p = fma(p, w, SAM_DIGAMMA_SEL(0.9510558760318328, 0.9227843350984671, 1.7061176684318005, 0.08333333333333287));
/* END GENERATED DIGAMMA */
/* psi(y + yl), y >= 1 (+inf included), |yl| <= ulp(y)/2 */
SA_FN double sam_digamma_2w(double y, double yl)
{
    const int k1 = y >= SAM_DIGAMMA_B2, k2 = y >= SAM_DIGAMMA_B3, k3 = y >= SAM_DIGAMMA_B4;
    const double iy = 1.0 / y;
    const double w = k3 ? iy * iy : y - (k2 ? SAM_DIGAMMA_C2 : (k1 ? SAM_DIGAMMA_C1 : SAM_DIGAMMA_C0));
    double p;
    SAM_DIGAMMA_HORNER(p, w);
    const double u = (y - SAM_PSI_X0_HI) + (yl - SAM_PSI_X0_LO);                 /* (y - hi: exact on [1, 2]) */
    const double d1 = iy * fma(iy, fma(iy, 1.0 / 6.0, 0.5), 1.0);                /* psi'(y) to 1 %: what yl moves */
    const double asym = (sa_log(y) - 0.5 * iy) - w * p;
    return k1 ? fma(yl, d1, k3 ? asym : p) : u * p;
}

SA_FN double sa_digamma(double x)
{
    if (!(x == x)) return x;
    if (x == SAM_INF) return x;
    const int neg = !(x > 0.0);
    if (neg && (x == -SAM_INF || floor(x) == x)) return SAM_NAN;                 /* the poles 0, -1, -2, ... */
    if (fabs(x) < 1.3877787807814457e-17) return -1.0 / x;                       /* 2^-56: psi(x) = -1/x - gamma_E + ... */
    const int shift = neg || x < SAM_DIGAMMA_B1;
    double y, sub = 0.0, subl = 0.0;
    const double yl = sam_two_sum(shift ? 1.0 : 0.0, neg ? -x : x, &y);
    if (neg) {                                   /* psi(x) = psi(1 - x) - pi cot(pi x), the cotangent term in two words */
        double sn, cs;
        sam_sincospi(x, &sn, &cs);
        const double q = cs / sn;
        const double ql = fma(-q, sn, cs) / sn;
        sub = q * SAM_GPI_HI;
        subl = fma(q, SAM_GPI_HI, -sub) + fma(q, SAM_GPI_LO, ql * SAM_GPI_HI);
    } else if (shift) sub = 1.0 / x;
    return (sam_digamma_2w(y, yl) - sub) - subl;
}

/* ---- trigamma ---- */
#define SAM_TRIGAMMA_B1 1.0      /* below: psi' x = psi'(x + 1) + 1/x^2 */
#define SAM_TRIGAMMA_B2 2.0
#define SAM_TRIGAMMA_B3 4.0
#define SAM_TRIGAMMA_B4 8.0      /* from here on: (1 + 1/(2y) + T(1/y^2)/y^2) / y */
#define SAM_TRIGAMMA_SEL(c0, c1, c2, c3) (k2 ? (k3 ? (c3) : (c2)) : (k1 ? (c1) : (c0)))
/* BEGIN GENERATED TRIGAMMA (tools/make_sa_math_coeffs.py) */
    /* coefficients by piece (zero above a piece's own degree); one Horner chain of degree 24
       piece 0: psi'(y), y = c + w, c = 1.5, y in [1.0, 2.0]: degree 24, error 2^-53.4
       piece 1: psi'(y), y = c + w, c = 3.0, y in [2.0, 4.0]: degree 24, error 2^-53.0
       piece 2: psi'(y), y = c + w, c = 6.0, y in [4.0, 8.0]: degree 24, error 2^-54.7
       piece 3: T = (y psi'(y) - 1 - 1/(2y))/w, w = 1/y^2 in [0, 0.015625]: degree 6, error 2^-58.8 (of the function's value) */
#define SAM_TRIGAMMA_C0 1.5
#define SAM_TRIGAMMA_C1 3.0
#define SAM_TRIGAMMA_C2 6.0
#define SAM_TRIGAMMA_HORNER(p, w) \
    p = SAM_TRIGAMMA_SEL(0.0014459090369969415, 2.1554277645795407e-11, 3.258943369835491e-19, 0.0); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(-0.0020870720089157142, -6.223248406952465e-11, -1.886393097947148e-18, 0.0)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(0.0007486890148235593, 4.469814621734972e-11, 2.759736922213069e-18, 0.0)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(-0.0010668064559446603, -1.274515415140973e-10, -1.5832187441984396e-17, 0.0)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(0.0030690965464267115, 7.329382334190199e-10, 1.8030462728058576e-16, 0.0)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(-0.004389290687344111, -2.0975820552374793e-09, -1.0373175519197836e-15, 0.0)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(0.00564467415342075, 5.400451053570852e-09, 5.389286865962702e-15, 0.0)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(-0.008019768440309974, -1.5361948569241443e-08, -3.088863223967219e-14, 0.0)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(0.011516140812509243, 4.417815234944036e-08, 1.790842951635376e-13, 0.0)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(-0.016259614773567462, -1.249833319023168e-07, -1.023331835281704e-12, 0.0)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(0.022841637462877776, 3.520335545610047e-07, 5.8314082257555344e-12, 0.0)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(-0.031984295171159555, -9.891519121723088e-07, -3.320703892819638e-11, 0.0)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(0.044566667766407414, 2.768731295610908e-06, 1.8876402723945843e-10, 0.0)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(-0.06174052097958386, -7.716440576044386e-06, -1.0709173349909197e-09, 0.0)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(0.08496878809335849, 2.140521000450944e-05, 6.063640912305573e-09, 0.0)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(-0.11604071812233813, -5.907353718802338e-05, -3.426270688127973e-08, 0.0)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(0.1570532019993859, 0.00016211365053690304, 1.9319123941109563e-07, 0.0)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(-0.21030987328212136, -0.00044214260916182864, -1.0869231313854683e-06, 0.0)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(0.27808081332751206, 0.0011977433855981318, 6.101330241719244e-06, 0.8586880107331692)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(-0.3621493650206583, -0.003220664291501515, -3.416912907097418e-05, -0.24699740954161503)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(0.46306452510150453, 0.008590309922246098, 0.00019089623483143874, 0.07569481310235808)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(-0.5790416377779077, -0.02271102057348086, -0.001063865223685503, -0.03333299706371194)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(0.7045455170012186, 0.05946970113341457, 0.005913914096377537, 0.023809522943893217)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(-0.8287966442343199, -0.15411380631918856, -0.03278973224511449, -0.03333333333249287)); \
    p = fma(p, w, SAM_TRIGAMMA_SEL(0.9348022005446793, 0.39493406684822646, 0.18132295573711532, 0.16666666666666655));
/* END GENERATED TRIGAMMA */
/* psi'(y + yl), y >= 1 (+inf included), |yl| <= ulp(y)/2 */
SA_FN double sam_trigamma_2w(double y, double yl)
{
    const int k1 = y >= SAM_TRIGAMMA_B2, k2 = y >= SAM_TRIGAMMA_B3, k3 = y >= SAM_TRIGAMMA_B4;
    const double iy = 1.0 / y;
    const double w = k3 ? iy * iy : y - (k2 ? SAM_TRIGAMMA_C2 : (k1 ? SAM_TRIGAMMA_C1 : SAM_TRIGAMMA_C0));
    double p;
    SAM_TRIGAMMA_HORNER(p, w);
    const double d2 = -(iy * iy) * fma(iy, fma(iy, 0.5, 1.0), 1.0);              /* psi''(y) to 2 %: what yl moves */
    /* 1/y + (1/(2y) + w T)/y, with what the rounding of 1/y lost */
    const double asym = iy + fma(iy, fma(w, p, 0.5 * iy), iy * fma(-iy, y, 1.0));
    return fma(yl, d2, k3 ? asym : p);
}

SA_FN double sa_trigamma(double x)
{
    if (!(x == x)) return x;
    if (x == SAM_INF) return 0.0;
    const int neg = !(x > 0.0);
    if (neg && floor(x) == x) return (x == -SAM_INF) ? SAM_NAN : SAM_INF;        /* the poles 0, -1, -2, ... */
    if (fabs(x) < 7.450580596923828e-09) { const double r = 1.0 / x; return r * r; }     /* 2^-27: 1/x^2 + pi^2/6 + ... */
    const int shift = neg || x < SAM_TRIGAMMA_B1;
    double y;
    const double yl = sam_two_sum(shift ? 1.0 : 0.0, neg ? -x : x, &y);
    const double v = sam_trigamma_2w(y, yl);
    if (neg) {                                   /* psi'(x) = (pi / sin(pi x))^2 - psi'(1 - x) */
        double sn, cs;
        sam_sincospi(x, &sn, &cs);
        const double s2 = sn * sn, s2l = fma(sn, sn, -s2);
        const double q = SAM_GPISQ_HI / s2;
        return (q - v) + (fma(-q, s2, SAM_GPISQ_HI) + (SAM_GPISQ_LO - q * s2l)) / s2;
    }
    const double ix = 1.0 / x;
    return shift ? fma(ix, ix, v) : v;
}
#endif /* SA_MATH_GAMMA_H */
