/*
 * sa_math_inv.h -- deterministic inverse trigonometric / inverse hyperbolic functions and the error function.
 *
 * The second block of the math library of the generated callbacks: sunode_amd/symode/codegen.py embeds this text
 * AFTER csrc/sa_math.h, and only into the header of a problem whose right-hand side (or one of its derivatives) calls
 * sa_asin / sa_acos / sa_atan / sa_atan2 / sa_asinh / sa_acosh / sa_atanh / sa_erf / sa_erfc -- the headers of all
 * other problems keep their text, and with it their cache keys and code objects.  Same contract as sa_math.h: ONE
 * sequence of IEEE-754 operations (+, -, *, /, sqrt, fabs, explicit fma(), integer bit operations, and sa_exp /
 * sa_log1p of the first block), compiled by hipcc for gfx950 and by gcc for the oracle with -ffp-contract=off, so the
 * device's values are the host's bit for bit.  No libm / ocml call, no table in memory.
 *
 * Intervals without divergence: a function with several approximation intervals (the argument reduction of the
 * arctangent, the pieces of the error function, small / large arguments of the inverse hyperbolic functions) selects
 * its coefficients and offsets with ternaries (v_cndmask on the device) and then runs ONE polynomial evaluation; only
 * the special-value exits branch.  The interval boundaries are the SAM_<FN>_B<k> definitions below
 * (codegen.math_inv_boundaries() reads them for the tests).
 *
 * Coefficients: tools/make_sa_math_coeffs.py (Chebyshev-node fits with mpmath at 120 digits; the fit interval and
 * the measured error of the rounded polynomial stand beside every set).  `--check` compares this file with its output.
 *
 * Accuracy (tests/test_inverse_erf_math.py, against mpmath at 200 bits; worst case measured over the test's ranges,
 * ceiling 4 ulp for every function):
 *   asin 0.57, acos 0.73, atan 0.63, atan2 0.97, asinh 1.05, acosh 1.26, atanh 1.52, erf 0.67, erfc 2.95 ulp.
 * The complementary error function keeps its relative accuracy down to the smallest normal result (x about 26.54):
 * x^2 enters sa_exp as a high and a low part; subnormal results are within one subnormal step.
 *
 * Special values (C99 Annex F): asin / acos outside [-1, 1], acosh below 1 and atanh beyond +-1 return NaN -- a
 * non-finite output makes the callback report a recoverable error, the path the logarithm of a negative state takes;
 * acos 1 = +0; atan +-inf = +-pi/2; atan2 follows the zero / infinity / sign table; atanh +-1 = +-inf; erf +-inf =
 * +-1, erfc -inf = 2, erfc +inf = +0; NaN in, NaN out; asin, atan, asinh, atanh and erf return -0.0 for -0.0.
 */
#ifndef SA_MATH_INV_H
#define SA_MATH_INV_H
#define SA_HAVE_MATH_INV 1

/* BEGIN GENERATED CONST (tools/make_sa_math_coeffs.py) */
#define SAM_ATAN_HALF_HI 0.4636476090008061
#define SAM_ATAN_HALF_LO 2.2698777452961687e-17
#define SAM_PIO4_HI 0.7853981633974483
#define SAM_PIO4_LO 3.061616997868383e-17
#define SAM_ATAN_3HALF_HI 0.982793723247329
#define SAM_ATAN_3HALF_LO 1.3903311031230998e-17
#define SAM_PI_HI 3.141592653589793
#define SAM_PI_LO 1.2246467991473532e-16
#define SAM_3PIO4 2.356194490192345
#define SAM_LN2 0.6931471805599453
/* END GENERATED CONST */
#define SAM_SIGN_BIT 0x8000000000000000ULL
/* |v| with the sign of s */
SA_FN double sam_copysign(double v, double s)
{
    return sam_from_bits((sam_bits(v) & ~SAM_SIGN_BIT) | (sam_bits(s) & SAM_SIGN_BIT));
}

/* ---- atan / atan2 ---- */
#define SAM_ATAN_B1 0.4375
#define SAM_ATAN_B2 0.6875
#define SAM_ATAN_B3 1.1875
#define SAM_ATAN_B4 2.4375
/* atan a for a >= 0 (+inf included; NaN passes through).  Reduction by interval of a:
     [0, 7/16)       t = a                         atan a = atan t
     [7/16, 11/16)   t = (2a - 1) / (a + 2)        atan(1/2) + atan t
     [11/16, 19/16)  t = (a - 1) / (a + 1)         pi/4 + atan t
     [19/16, 39/16)  t = (a - 3/2) / (3a/2 + 1)    atan(3/2) + atan t
     [39/16, inf)    t = -1 / a                    pi/2 + atan t
   as ONE quotient t = (n1 a + n0) / (d1 a + d0) with selected coefficients, |t| <= 7/16, and one polynomial */
SA_FN double sam_atan_pos(double a)
{
    a = (a > 1e300) ? 1e300 : a;                 /* (-1 / a is below half an ulp of pi/2 long before) */
    const int i1 = a >= SAM_ATAN_B1, i2 = a >= SAM_ATAN_B2, i3 = a >= SAM_ATAN_B3, i4 = a >= SAM_ATAN_B4;
    const double n1 = i4 ? 0.0 : (i2 ? 1.0 : (i1 ? 2.0 : 1.0));
    const double n0 = i4 ? -1.0 : (i3 ? -1.5 : (i1 ? -1.0 : 0.0));
    const double d1 = i4 ? 1.0 : (i3 ? 1.5 : (i1 ? 1.0 : 0.0));
    const double d0 = i4 ? 0.0 : (i2 ? 1.0 : (i1 ? 2.0 : 1.0));
    const double hi = i4 ? SAM_PIO2_1 : (i3 ? SAM_ATAN_3HALF_HI : (i2 ? SAM_PIO4_HI : (i1 ? SAM_ATAN_HALF_HI : 0.0)));
    const double lo = i4 ? SAM_PIO2_2 : (i3 ? SAM_ATAN_3HALF_LO : (i2 ? SAM_PIO4_LO : (i1 ? SAM_ATAN_HALF_LO : 0.0)));
    const double t = fma(a, n1, n0) / fma(a, d1, d0);
    const double z = t * t;
    /* BEGIN GENERATED ATAN (tools/make_sa_math_coeffs.py) */
    /* P(z) = (t - atan t) / t^3, z = t^2 in [0, (7/16)^2]: degree 11, error 2^-57.9 */
    double p = -0.014773184616983806;
    p = fma(p, z, 0.033128134256069586);
    p = fma(p, z, -0.04492259293193656);
    p = fma(p, z, 0.05216679739313656);
    p = fma(p, z, -0.05876946456755061);
    p = fma(p, z, 0.06666241923359964);
    p = fma(p, z, -0.07692285554889286);
    p = fma(p, z, 0.09090908355602592);
    p = fma(p, z, -0.11111111096645038);
    p = fma(p, z, 0.14285714285566806);
    p = fma(p, z, -0.1999999999999941);
    p = fma(p, z, 0.3333333333333333);
    /* END GENERATED ATAN */
    return hi - ((t * z * p - lo) - t);
}

SA_FN double sa_atan(double x) { return sam_copysign(sam_atan_pos(fabs(x)), x); }

SA_FN double sa_atan2(double y, double x)
{
    if (!(x == x) || !(y == y)) return x + y;
    const double ax = fabs(x), ay = fabs(y);
    const int neg = (int)(sam_bits(x) >> 63);
    if (ay == SAM_INF) return sam_copysign((ax == SAM_INF) ? (neg ? SAM_3PIO4 : SAM_PIO4_HI) : SAM_PIO2_1, y);
    if (ax == 0.0) return sam_copysign((ay == 0.0) ? (neg ? SAM_PI_HI : 0.0) : SAM_PIO2_1, y);
    const double z = sam_atan_pos(ay / ax);      /* (ax = inf: the quotient is 0) */
    return sam_copysign(neg ? (SAM_PI_HI - z) + SAM_PI_LO : z, y);
}

/* ---- asin / acos ---- */
#define SAM_ASIN_B1 0.5
#define SAM_ACOS_B1 0.5
/* a = |x| < 1 -> s, r = asin(s)/s - 1 and sl, with
     a < 1/2:   s = a, sl = 0                            asin a = s + s r
     a >= 1/2:  s + sl = sqrt((1 - a) / 2) (sl: what the rounding of the square root lost)
                                                         asin a = pi/2 - 2 (s + sl + s r)
   returns a >= 1/2 */
SA_FN int sam_asin_reduce(double a, double *s_out, double *r_out, double *sl_out)
{
    const int big = a >= SAM_ASIN_B1;
    const double z = big ? 0.5 * (1.0 - a) : a * a;
    const double s = big ? sqrt(z) : a;
    /* BEGIN GENERATED ASIN (tools/make_sa_math_coeffs.py) */
    /* Q(z) = (asin s - s) / s^3, z = s^2 in [0, 1/4]: degree 13, error 2^-58.6 */
    double q = 0.02961201126495512;
    q = fma(q, z, -0.01924167174674304);
    q = fma(q, z, 0.019554513336123378);
    q = fma(q, z, 0.0030448799094556773);
    q = fma(q, z, 0.009319560794767446);
    q = fma(q, z, 0.009621842970100282);
    q = fma(q, z, 0.011566459612121669);
    q = fma(q, z, 0.01396378001220357);
    q = fma(q, z, 0.017352816540325496);
    q = fma(q, z, 0.02237215744350722);
    q = fma(q, z, 0.03038194447553234);
    q = fma(q, z, 0.044642857142551895);
    q = fma(q, z, 0.07500000000000118);
    q = fma(q, z, 0.16666666666666666);
    /* END GENERATED ASIN */
    *s_out = s;
    *r_out = z * q;
    *sl_out = big ? fma(-s, s, z) / (2.0 * s) : 0.0;
    return big;
}

SA_FN double sa_asin(double x)
{
    const double a = fabs(x);
    if (!(a < 1.0)) return (a == 1.0) ? sam_copysign(SAM_PIO2_1, x) : SAM_NAN;
    double s, r, sl;
    const int big = sam_asin_reduce(a, &s, &r, &sl);
    const double t1 = SAM_PIO2_1 - 2.0 * s;
    const double e = (SAM_PIO2_1 - t1) - 2.0 * s;                /* exact: pi/2 > 2 s */
    const double vb = t1 + (e + (SAM_PIO2_2 - 2.0 * fma(s, r, sl)));
    return sam_copysign(big ? vb : fma(a, r, a), x);
}

SA_FN double sa_acos(double x)
{
    const double a = fabs(x);
    if (!(a < 1.0)) return (x == 1.0) ? 0.0 : ((x == -1.0) ? SAM_PI_HI : SAM_NAN);
    double s, r, sl;
    const int big = sam_asin_reduce(a, &s, &r, &sl);
    /* |x| < 1/2: pi/2 - (x + x r);  x >= 1/2: w = 2 (s + sl + s r);  x <= -1/2: pi - w */
    const double vs = SAM_PIO2_1 - (x - (SAM_PIO2_2 - x * r));
    const double wh = 2.0 * s, wl = 2.0 * fma(s, r, sl);
    const double t1 = SAM_PI_HI - wh;
    const double e = (SAM_PI_HI - t1) - wh;                      /* exact: pi > w */
    const double vb = (x < 0.0) ? t1 + (e + (SAM_PI_LO - wl)) : wh + wl;
    return big ? vb : vs;
}

/* ---- asinh / acosh / atanh: on sa_log1p ---- */
#define SAM_ASINH_B1 3.273390607896142e+150      /* 2^500: beyond it a^2 is not formed, asinh a = ln a + ln 2 */
#define SAM_ACOSH_B1 3.273390607896142e+150
#define SAM_ATANH_B1 0.5
SA_FN double sa_asinh(double x)
{
    const double a = fabs(x);
    const int big = a >= SAM_ASINH_B1;
    const double t = a * a;
    const double w = a + t / (1.0 + sqrt(1.0 + t));              /* asinh a = ln(1 + w) */
    const double v = sa_log1p(big ? a : w) + (big ? SAM_LN2 : 0.0);
    return sam_copysign(v, x);
}

SA_FN double sa_acosh(double x)
{
    if (!(x >= 1.0)) return SAM_NAN;
    const int big = x >= SAM_ACOSH_B1;
    const double t = x - 1.0;
    const double w = t + sqrt(fma(t, t, 2.0 * t));               /* acosh x = ln(1 + w) */
    return sa_log1p(big ? x : w) + (big ? SAM_LN2 : 0.0);
}

SA_FN double sa_atanh(double x)
{
    const double a = fabs(x);
    if (!(a < 1.0)) return (a == 1.0) ? sam_copysign(SAM_INF, x) : SAM_NAN;
    /* atanh a = ln(1 + w) / 2, w = 2a / (1 - a), formed as 2a + 2a^2 / (1 - a) below 1/2 (1 - a is exact from there on) */
    const int small = a < SAM_ATANH_B1;
    const double a2 = 2.0 * a;
    const double q = (small ? a2 * a : a2) / (1.0 - a);
    return sam_copysign(0.5 * sa_log1p(small ? a2 + q : q), x);
}

/* ---- erf / erfc ---- */
#define SAM_ERF_B1 1.0
#define SAM_ERF_B2 1.5
#define SAM_ERF_B3 2.5
#define SAM_ERF_B4 4.0
#define SAM_ERF_B5 8.0
#define SAM_ERFC_B0 -1.0         /* erfc x = 1 - erf x on (-1, 1/2), from the scaled pieces outside */
#define SAM_ERFC_B1 0.5
#define SAM_ERFC_CLAMP 27.5      /* exp(-27.5^2) is below half the smallest subnormal */
#define SAM_ERF_SEL(c0, c1, c2, c3, c4, c5) (k4 ? (k5 ? (c5) : (c4)) : (k2 ? (k3 ? (c3) : (c2)) : (k1 ? (c1) : (c0))))
/* BEGIN GENERATED ERF (tools/make_sa_math_coeffs.py) */
    /* coefficients by piece (zero above a piece's own degree); one Horner chain of degree 17
       piece 0: E(z) = erf(s)/s - 1, z = s^2 in [0, 1.0]: degree 12, error 2^-55.5
       piece 1: erfcx(c + w), c = 1.0, a in [0.5, 1.5]: degree 17, error 2^-56.0
       piece 2: erfcx(c + w), c = 2.0, a in [1.5, 2.5]: degree 15, error 2^-54.5
       piece 3: erfcx(c + w), c = 3.25, a in [2.5, 4.0]: degree 16, error 2^-55.9
       piece 4: a erfcx(a) at 1/a^2 = c + w, c = 0.0390625, a in [4.0, 8.0]: degree 12, error 2^-54.2
       piece 5: a erfcx(a) at 1/a^2 = c + w, c = 0.008473657024793389, a in [8.0, 27.5]: degree 9, error 2^-55.1 */
#define SAM_ERF_C1 1.0
#define SAM_ERF_C2 2.0
#define SAM_ERF_C3 3.25
#define SAM_ERF_C4 0.0390625
#define SAM_ERF_C5 0.008473657024793389
#define SAM_ERF_HORNER(p, w) \
    p = SAM_ERF_SEL(0.0, -3.914617199714194e-08, 0.0, 0.0, 0.0, 0.0); \
    p = fma(p, w, SAM_ERF_SEL(0.0, 1.3784633743013745e-07, 0.0, 1.49801892689003e-11, 0.0, 0.0)); \
    p = fma(p, w, SAM_ERF_SEL(0.0, -4.299143543295316e-07, -6.2369421691116115e-09, -7.42679319093461e-11, 0.0, 0.0)); \
    p = fma(p, w, SAM_ERF_SEL(0.0, 1.4340410570175926e-06, 2.4838591176738408e-08, 3.2681718268240385e-10, 0.0, 0.0)); \
    p = fma(p, w, SAM_ERF_SEL(0.0, -4.675888436513413e-06, -9.059144499761123e-08, -1.5652413273818979e-09, 0.0, 0.0)); \
    p = fma(p, w, SAM_ERF_SEL(5.957176147748911e-11, 1.4754609192515983e-05, 3.4423946450209766e-07, 7.4072185561795875e-09, 533648.984327875, 0.0)); \
    p = fma(p, w, SAM_ERF_SEL(-1.1372848856791674e-09, -4.5143861219947744e-05, -1.2795531726707594e-06, -3.429349515414528e-08, -84070.76899544074, 0.0)); \
    p = fma(p, w, SAM_ERF_SEL(1.4659775274047436e-08, 0.0001336627622717746, 4.628306339064563e-06, 1.558809412663323e-07, 13059.00181471106, 0.0)); \
    p = fma(p, w, SAM_ERF_SEL(-1.6350312701054695e-07, -0.00038195453301478085, -1.6293715542527493e-05, -6.952069862447502e-07, -2339.105886488694, -18216.578552578376)); \
    p = fma(p, w, SAM_ERF_SEL(1.6461000484121368e-06, 0.0010502694181821256, 5.5728299853060465e-05, 3.0388320233539232e-06, 451.4394467707696, 2462.7025503433947)); \
    p = fma(p, w, SAM_ERF_SEL(-1.4925595266831182e-05, -0.002769064775600966, -0.00018477836740122568, -1.3004640448437801e-05, -94.69585436409021, -369.8315471404554)); \
    p = fma(p, w, SAM_ERF_SEL(0.0001205533111164271, 0.0069701423740626415, 0.000592469996313369, 5.442040880902426e-05, 21.97220276864858, 63.67249480346449)); \
    p = fma(p, w, SAM_ERF_SEL(-0.000854832698083379, -0.0166618690904203, -0.0018316642757311742, -0.00022238256955206057, -5.761704168019539, -12.769414853907596)); \
    p = fma(p, w, SAM_ERF_SEL(0.0052239776248180145, 0.03757229621531269, 0.00544073853744156, 0.0008860045775344011, 1.7608315396927912, 3.08402698729616)); \
    p = fma(p, w, SAM_ERF_SEL(-0.026866170645076792, -0.07922696894132669, -0.015460637764291092, -0.003435471300908234, -0.6575783773547513, -0.9433065591410376)); \
    p = fma(p, w, SAM_ERF_SEL(0.11283791670954879, 0.15437156137190824, 0.041802752603526915, 0.012937290883018157, 0.32551774975812436, 0.39775078276265285)); \
    p = fma(p, w, SAM_ERF_SEL(-0.3761263890318375, -0.27321201478389856, -0.1067964618534896, -0.04719940232117037, -0.2531516745214893, -0.275142935427954)); \
    p = fma(p, w, SAM_ERF_SEL(0.1283791670955126, 0.427583576155807, 0.25539567631050575, 0.16633534842682188, 0.5537602328010941, 0.5618289666135186));
/* END GENERATED ERF */
/* a = |x|.  first != 0 (a < 1): returns E(a^2), erf a = a + a E.  Otherwise (a >= 1/2) returns erfc a =
   exp(-a^2) erfcx(a), erfcx from the piece of a: a polynomial in a - c below 4, (1/a) times a polynomial in
   1/a^2 - c from there on; a^2 = h + l exactly, exp(-a^2) = exp(-h) (1 - l) */
SA_FN double sam_erf_core(double a, int first)
{
    const double ac = (a > SAM_ERFC_CLAMP) ? SAM_ERFC_CLAMP : a;
    const int k1 = !first, k2 = ac >= SAM_ERF_B2, k3 = ac >= SAM_ERF_B3, k4 = ac >= SAM_ERF_B4, k5 = ac >= SAM_ERF_B5;
    const double h = ac * ac, l = fma(ac, ac, -h);
    const double s = 1.0 / ac;
    const double w = k4 ? s * s - (k5 ? SAM_ERF_C5 : SAM_ERF_C4)
                        : (k1 ? ac - (k3 ? SAM_ERF_C3 : (k2 ? SAM_ERF_C2 : SAM_ERF_C1)) : h);
    double p;
    SAM_ERF_HORNER(p, w);
    const double e = sa_exp(-h);
    return k1 ? (k4 ? s * p : p) * fma(e, -l, e) : p;
}

SA_FN double sa_erf(double x)
{
    const double a = fabs(x);
    const int first = a < SAM_ERF_B1;
    const double v = sam_erf_core(a, first);
    return first ? fma(x, v, x) : sam_copysign(1.0 - v, x);
}

SA_FN double sa_erfc(double x)
{
    const double a = fabs(x);
    const int first = x > SAM_ERFC_B0 && x < SAM_ERFC_B1;
    const double v = sam_erf_core(a, first);
    return first ? 1.0 - fma(x, v, x) : ((x < 0.0) ? 2.0 - v : v);
}
#endif /* SA_MATH_INV_H */
