/*
 * sa_math_bessel.h -- deterministic Bessel functions of integer order: J_n, Y_n, I_n, K_n, 0 <= n <= SAM_BESSEL_NMAX.
 *
 * The fourth block of the math library of the generated callbacks: sunode_amd/symode/codegen.py embeds this text AFTER
 * csrc/sa_math.h (and after csrc/sa_math_inv.h / csrc/sa_math_gamma.h where those are present), and only into the
 * header of a problem whose right-hand side (or one of its derivatives) calls sa_bessel_j / sa_bessel_y / sa_bessel_i /
 * sa_bessel_k -- the headers of all other problems keep their text, and with it their cache keys and code objects.
 * Same contract as sa_math.h and sa_math_gamma.h: ONE sequence of IEEE-754 operations (+, -, *, /, sqrt, fabs,
 * explicit fma(), integer bit operations, and sa_exp / sa_log and the kernels sam_rem_pio2 / sam_sin_k / sam_cos_k of
 * the first block), compiled by hipcc for gfx950 and by gcc for the oracle with -ffp-contract=off, so the device's
 * values are the host's bit for bit.  No libm / ocml call, no table in memory.  The order n is an integer literal in
 * every generated call: the loops below have trip counts that depend on n alone (or on nothing), never on x.
 *
 * Orders 0 and 1.  The piece of x is selected with ternaries (v_cndmask on the device) and ONE Horner chain per
 * function runs on the selected coefficients; the piece boundaries are the SAM_<FN>_B<k> definitions below
 * (codegen.math_bessel_boundaries() reads them for the tests).
 *   J0, J1   below 8: polynomials in x - c; the piece that holds the first zero z (2.4048 / 3.8317) is fitted as
 *            J(x) / (x - z) and multiplied by (x - z_hi) - z_lo, so the zero keeps its relative accuracy; J1's first
 *            piece is x P(x).  From 8 on: sqrt(2 / (pi x)) (P cos chi - Q sin chi), chi = x - pi/4 - n pi/2, P and Q as
 *            chains in 1/x - c.
 *   Y0, Y1   below 1/2: (2/pi) ln x J(x) + even series (- (2/pi)/x for Y1), the products of ln x in short polynomials
 *            of x^2; up to 8: polynomials in x - c, the first zero (0.8936 / 2.1971) factored out as for J; from 8 on
 *            sqrt(2 / (pi x)) (P sin chi + Q cos chi) with the P of the own chain and the Q chain of J.
 *   I0, I1   below 8: the (positive) series in x^2; beyond: sqrt(x) exp(-x) I(x) as a chain in 1/x - c, times
 *            exp(x) / sqrt(x); above 700 the exponential is taken of x - 32 and the result multiplied by a two-word
 *            exp(32), so that I reaches its own overflow threshold (713.98...), not exp's.
 *   K0, K1   below 1: -ln x I0(x) + series, 1/x + ln x I1(x) + series; beyond: sqrt(x) exp(x) K(x) as a chain in
 *            1/x - c, times exp(-x) / sqrt(x).  The factor exp(-x) is applied LAST, after the recurrence of a higher
 *            order, so a subnormal result is rounded once and K underflows to +0 where it must.
 * sin chi and cos chi: x is reduced modulo pi/2 by sam_rem_pio2 (three-word pi/2, two-word remainder r); pi/4 is
 * subtracted from (r >= 0) or added to (r < 0, one quadrant down) the REMAINDER in two words, which leaves it in
 * [-pi/4, pi/4], and sam_sin_k / sam_cos_k are evaluated once there; the quadrant (shifted by n) picks and signs them.
 * No sum cos x + sin x that cancels is formed, and never sa_sin(x - const).  Beyond the domain of sa_sin (|x| > 2^50) J
 * and Y return NaN, as sa_sin does (+0 at +inf).
 *
 * Orders n >= 2.
 *   Y, K     upward recurrence from the orders 0 and 1 (stable for both).
 *   J        |x| >= n: upward recurrence from J0 and J1.  1 <= |x| < n (where that is unstable): Miller's downward
 *            recurrence from order 3n + SAM_JN_EXTRA, normalised by the Neumann sum J0 + 2 (J2 + J4 + ...) = 1 -- not
 *            by J0 itself, which has three zeros below 9.  |x| < 1: the power series, SAM_BESSEL_SERIES terms.
 *   I        1 <= |x| < SAM_IN_B2: Miller's downward recurrence from order SAM_IN_START, normalised by I0 (all terms
 *            positive).  |x| < 1: the power series.  From SAM_IN_B2 on, where a downward recurrence of fixed length no
 *            longer converges: Hankel's asymptotic series, SAM_IN_TERMS terms whose coefficients depend on n only.
 *            The upward recurrence is not used for I.
 * Only the special-value exits, the choice of method for an order >= 2 (series / downward / upward or asymptotic) and
 * the special-value exits of sa_exp / sa_log branch.  There is no loop with a data-dependent trip count.
 *
 * Coefficients: tools/make_sa_math_coeffs.py (Chebyshev-node fits with mpmath at 120 digits; the fit interval and the
 * measured error of the rounded polynomial stand beside every set).  `--check` compares this file with its output.
 * The "error 2^-x" figures below are measured at 201 equidistant points of the fit interval, not at the 1 001 of the
 * other blocks (the functions are expensive at that precision), and the degree is searched in steps of four and then
 * downwards: compare them across headers with that in mind.  The check that counts is the test's, below.
 *
 * Accuracy (tests/test_bessel_math.py, against mpmath at 200 bits; worst case over the test's seeded sample of 1 500
 * points per range).  I and K: in ulp of the result.  J and Y: in ulp of the result below the function's first zero,
 * beyond it in units of spacing(M_n(x)), M_n = sqrt(J_n^2 + Y_n^2) -- next to a later zero the result is accurate
 * relative to the envelope, not to itself.  Ceiling for the orders 0 and 1: 4.  Measured (order 0 / 1 / 2 / 5 / 9):
 *   J   0.57 / 0.93 / 1.06 / 2.19 / 3.20 over 1e-300 .. 1;  2.78 / 2.28 / 4.56 / 30.8 / 74.8 on (0, 50);
 *       2.31 / 2.15 / 2.34 / 2.46 / 2.57 on (50, 1e6);  2.28 / 1.97 / 2.32 / 2.09 / 2.47 on (1e6, 2^50)
 *   Y   1.54 / 1.06 / 2.07 / 4.31 / 8.28 over 1e-300 .. 1;  2.10 / 2.67 / 11.0 / 440 / 95.1 on (0, 50);
 *       1.94 / 2.06 / 2.23 / 2.74 / 3.22 on (50, 1e6);  2.40 / 2.32 / 2.41 / 2.62 / 2.59 on (1e6, 2^50)
 *   I   0.50 / 1.17 / 1.78 / 2.04 / 2.82 over 1e-300 .. 1;  2.73 / 2.92 / 3.60 / 5.14 / 8.75 on (0, 30);
 *       2.74 / 2.69 / 2.89 / 3.07 / 3.45 on (30, 713)
 *   K   1.44 / 0.92 / 2.00 / 5.28 / 8.13 over 1e-300 .. 1;  2.60 / 3.02 / 2.68 / 3.66 / 6.09 on (0, 30);
 *       2.69 / 3.29 / 2.97 / 3.79 / 3.90 on (30, 745)
 * The large figures of J_n and Y_n, n >= 2, on (0, 50) are single points next to the FIRST zero of the function, on
 * its lower side, where the unit is the ulp of the (small) result: a recurrence from the orders 0 and 1 is accurate
 * relative to the envelope M_n there as everywhere else, not relative to a value that vanishes.  Beyond the first
 * zero the same orders stay within 2.35 / 2.60 / 3.56 (J) and 2.45 / 2.93 / 3.27 (Y) envelope units on (0, 50).  The
 * ceilings of the orders >= 2 in the test are these figures times 1.5, rounded up, (0, 50) split at the first zero.
 *
 * Special values: NaN in, NaN out.  x = +-0: J_0 = I_0 = 1, J_n = I_n = 0 for n >= 1 (with the sign of x for an odd n),
 * Y_n = -inf, K_n = +inf.  x < 0: J_n(-x) = (-1)^n J_n(x), I_n(-x) = (-1)^n I_n(x); Y and K are NaN.  +inf: J, Y, K +0,
 * I +inf (-inf: J (-1)^n 0, I (-1)^n inf).  I overflows to +inf above 713.98..., K underflows to +0 beyond 745; Y_n and K_n
 * overflow to -inf / +inf towards 0.  A non-finite output makes the callback report a recoverable error, the path the
 * logarithm of a negative state takes.
 */
#ifndef SA_MATH_BESSEL_H
#define SA_MATH_BESSEL_H
#define SA_HAVE_MATH_BESSEL 1
#define SAM_BESSEL_NMAX 9
#define SAM_BESSEL_XMAX 1125899906842624.0       /* 2^50: the domain of sam_rem_pio2 */
/* The four public functions are real functions on the device, never inlined into a callback: one call site of a
   right-hand side with its derivatives would otherwise carry every chain below several times over (the code object of
   a five-state model took 23 minutes to compile that way).  The helpers stay SA_FN: inlined into the four functions
   in the one-lane kernels (bdf_kernels.hip), real calls themselves in the lane-group, workgroup and memory-resident
   mappings (bdf_wave.hip, bdf_mem.hip), whose SA_FN is noinline for every callback helper.  The operation sequence,
   and with it every bit of the result, is the same in all of them. */
#ifdef __HIP__
#define SAM_BESSEL_FN static __device__ __attribute__((noinline))
#else
#define SAM_BESSEL_FN SA_FN
#endif

/* BEGIN GENERATED CONST (tools/make_sa_math_coeffs.py) */
#define SAM_BPIO4_HI 0.7853981633974483
#define SAM_BPIO4_LO 3.061616997868383e-17
#define SAM_BE32_HI 78962960182680.69
#define SAM_BE32_LO 0.007660978022635108
#define SAM_J0_Z_HI 2.404825557695773
#define SAM_J0_Z_LO -1.176691651530894e-16
#define SAM_J1_Z_HI 3.8317059702075125
#define SAM_J1_Z_LO -1.5269184090088067e-16
#define SAM_Y0_Z_HI 0.8935769662791675
#define SAM_Y0_Z_LO 2.6596231539720385e-17
#define SAM_Y1_Z_HI 2.197141326031017
#define SAM_Y1_Z_LO -4.8259835876454966e-17
#define SAM_BSQ2OPI 0.7978845608028654
#define SAM_B2OPI 0.6366197723675814
#define SAM_BISQ2PI 0.3989422804014327
/* END GENERATED CONST */

/* sin and cos of x - pi/4 for 0 <= x <= 2^50 */
SA_FN void sam_bessel_phase(double x, double *s_out, double *c_out)
{
    double r, rl;
    const int q = sam_rem_pio2(x, &r, &rl);
    const int neg = r < 0.0;
    const double ph = neg ? SAM_BPIO4_HI : -SAM_BPIO4_HI, pl = neg ? SAM_BPIO4_LO : -SAM_BPIO4_LO;
    const double h0 = r + ph;
    const double bb = h0 - r;
    const double e = (r - (h0 - bb)) + (ph - bb);                /* two-sum */
    const double lo = e + (rl + pl);
    const double h = h0 + lo;
    const double l = (h0 - h) + lo;
    const double s = sam_sin_k(h, l), c = sam_cos_k(h, l);
    const int k = (q - neg) & 3;                                 /* x - pi/4 = k pi/2 + (h + l) */
    const double sv = (k & 1) ? c : s, cv = (k & 1) ? s : c;
    *s_out = (k & 2) ? -sv : sv;
    *c_out = ((k + 1) & 2) ? -cv : cv;
}

/* ---- J0, J1 (x >= 0 finite, x <= 2^50; sn, cs: sin and cos of x - pi/4) ---- */
#define SAM_J0_B1 1.5
#define SAM_J0_B2 4.0
#define SAM_J0_B3 8.0            /* from here on: P, Q in 1/x */
#define SAM_J0_B4 16.0
#define SAM_J1_B1 1.5
#define SAM_J1_B2 5.0
#define SAM_J1_B3 8.0
#define SAM_J1_B4 16.0
/* (the SEL macros read the piece flags of the ENCLOSING scope) */
#define SAM_J0_SEL(c0, c1, c2, c3, c4) (k3 ? (k4 ? (c4) : (c3)) : (k2 ? (c2) : (k1 ? (c1) : (c0))))
#define SAM_J1_SEL(c0, c1, c2, c3, c4) SAM_J0_SEL(c0, c1, c2, c3, c4)
#define SAM_J0Q_SEL(c0, c1) (kq ? (c1) : (c0))
#define SAM_J1Q_SEL(c0, c1) (kq ? (c1) : (c0))
/* BEGIN GENERATED J0 (tools/make_sa_math_coeffs.py) */
    /* coefficients by piece (zero above a piece's own degree); one Horner chain of degree 19
       piece 0: J0(x), x = c + w, c = 0.75, x in [0.0, 1.5]: degree 14, error 2^-53.5
       piece 1: J0(x)/(x - z), z the first zero, x = c + w, c = 2.75, x in [1.5, 4.0]: degree 15, error 2^-55.6
       piece 2: J0(x), error relative to M0, x = c + w, c = 6.0, x in [4.0, 8.0]: degree 19, error 2^-52.7
       piece 3: P0, 1/x = c + w, c = 0.09375, x in [8.0, 16.0]: degree 10, error 2^-55.2
       piece 4: P0, 1/x = c + w, c = 0.03125, x in [16.0, inf]: degree 11, error 2^-54.8 */
#define SAM_J0_C0 0.75
#define SAM_J0_C1 2.75
#define SAM_J0_C2 6.0
#define SAM_J0_C3 0.09375
#define SAM_J0_C4 0.03125
#define SAM_J0_HORNER(p, w) \
    p = SAM_J0_SEL(0.0, 0.0, -5.78019104589415e-19, 0.0, 0.0); \
    p = fma(p, w, SAM_J0_SEL(0.0, 0.0, -2.443784554811447e-17, 0.0, 0.0)); \
    p = fma(p, w, SAM_J0_SEL(0.0, 0.0, 2.2413859522698786e-16, 0.0, 0.0)); \
    p = fma(p, w, SAM_J0_SEL(0.0, 0.0, 8.211482151731294e-15, 0.0, 0.0)); \
    p = fma(p, w, SAM_J0_SEL(0.0, -8.072785400854052e-15, -6.697687520203093e-14, 0.0, 0.0)); \
    p = fma(p, w, SAM_J0_SEL(-1.782095706624859e-12, 7.177939085072082e-14, -2.069112787688174e-12, 0.0, 0.0)); \
    p = fma(p, w, SAM_J0_SEL(-2.285405098012363e-11, 2.089032282768845e-12, 1.5645078700387465e-11, 0.0, 0.0)); \
    p = fma(p, w, SAM_J0_SEL(3.5325436224099185e-10, -1.6900970762113938e-11, 3.960774624845887e-10, 0.0, 0.0)); \
    p = fma(p, w, SAM_J0_SEL(3.8789961117651536e-09, -4.0484886328007423e-10, -2.7609585435688675e-09, 0.0, 345.45934959314604)); \
    p = fma(p, w, SAM_J0_SEL(-5.108057819702046e-08, 2.9457294122996634e-09, -5.51132199412778e-08, 14.271990554839244, 2.932282931531467)); \
    p = fma(p, w, SAM_J0_SEL(-4.660434587830095e-07, 5.7348087183581345e-08, 3.510618426627905e-07, 1.589041959221853, -19.43272387527625)); \
    p = fma(p, w, SAM_J0_SEL(5.137558799907031e-06, -3.7074492692633336e-07, 5.22718360499982e-06, -2.190031150713484, 2.4046934361387464)); \
    p = fma(p, w, SAM_J0_SEL(3.734429676429364e-05, -5.59221650372237e-06, -3.0037971984533896e-05, 0.6648371739199596, 1.177166184524856)); \
    p = fma(p, w, SAM_J0_SEL(-0.0003316456348620103, 3.164243669914435e-05, -0.00030597063486243056, 0.05811636073147282, -0.4261210687563326)); \
    p = fma(p, w, SAM_J0_SEL(-0.0017969137858305643, 0.00034294954778113913, 0.0015513507450481032, -0.15809607600117354, -0.09772588202361436)); \
    p = fma(p, w, SAM_J0_SEL(0.012110582845770232, -0.0016665108149023582, 0.009276407324868143, 0.0592936228873087, 0.1041510888841786)); \
    p = fma(p, w, SAM_J0_SEL(0.04330193429588791, -0.011338530635182162, -0.039367498300144674, 0.03449081277031494, 0.013679356117534496)); \
    p = fma(p, w, SAM_J0_SEL(-0.19929206946674952, 0.04618555079526836, -0.0983796168027956, -0.06496834811470363, -0.06966339443031938)); \
    p = fma(p, w, SAM_J0_SEL(-0.34924360217486217, 0.14357815179469602, 0.27668385812756563, -0.012836219732564122, -0.004380941795461027)); \
    p = fma(p, w, SAM_J0_SEL(0.8642422751666486, -0.4755318114307082, 0.15064525725099692, 0.9993903253726394, 0.9999314418780413));
/* END GENERATED J0 */
/* BEGIN GENERATED J0Q (tools/make_sa_math_coeffs.py) */
    /* coefficients by piece (zero above a piece's own degree); one Horner chain of degree 11
       piece 0: Q0, 1/x = c + w, c = 0.09375, x in [8.0, 16.0]: degree 10, error 2^-60.3
       piece 1: Q0, 1/x = c + w, c = 0.03125, x in [16.0, inf]: degree 11, error 2^-59.9 */
#define SAM_J0Q_C0 0.09375
#define SAM_J0Q_C1 0.03125
#define SAM_J0Q_HORNER(p, w) \
    p = SAM_J0Q_SEL(0.0, -122.76982142498352); \
    p = fma(p, w, SAM_J0Q_SEL(-16.78429754728655, 79.5684748768464)); \
    p = fma(p, w, SAM_J0Q_SEL(6.664266549281106, -4.226128704321189)); \
    p = fma(p, w, SAM_J0Q_SEL(-0.7658900445501032, -4.648622215687442)); \
    p = fma(p, w, SAM_J0Q_SEL(-0.5345713431127157, 1.0190950802870777)); \
    p = fma(p, w, SAM_J0Q_SEL(0.34539810881597954, 0.3222221200824507)); \
    p = fma(p, w, SAM_J0Q_SEL(-0.04749445356634296, -0.1943878918343999)); \
    p = fma(p, w, SAM_J0Q_SEL(-0.07157537679796475, -0.033726810991615695)); \
    p = fma(p, w, SAM_J0Q_SEL(0.05693255081715451, 0.07108017613446324)); \
    p = fma(p, w, SAM_J0Q_SEL(0.01894722600759973, 0.00679820379248161)); \
    p = fma(p, w, SAM_J0Q_SEL(-0.12314938419955022, -0.12478649514502368)); \
    p = fma(p, w, SAM_J0Q_SEL(-0.011659946539503769, -0.0039040215445614256));
/* END GENERATED J0Q */
/* BEGIN GENERATED J1 (tools/make_sa_math_coeffs.py) */
    /* coefficients by piece (zero above a piece's own degree); one Horner chain of degree 17
       piece 0: J1(x)/x, x = c + w, c = 0.75, x in [0.0, 1.5]: degree 13, error 2^-53.7
       piece 1: J1(x)/(x - z), z the first zero, x = c + w, c = 3.25, x in [1.5, 5.0]: degree 16, error 2^-53.8
       piece 2: J1(x), error relative to M1, x = c + w, c = 6.5, x in [5.0, 8.0]: degree 17, error 2^-52.4
       piece 3: P1, 1/x = c + w, c = 0.09375, x in [8.0, 16.0]: degree 10, error 2^-55.4
       piece 4: P1, 1/x = c + w, c = 0.03125, x in [16.0, inf]: degree 11, error 2^-53.2 */
#define SAM_J1_C0 0.75
#define SAM_J1_C1 3.25
#define SAM_J1_C2 6.5
#define SAM_J1_C3 0.09375
#define SAM_J1_C4 0.03125
#define SAM_J1_HORNER(p, w) \
    p = SAM_J1_SEL(0.0, 0.0, 4.935328950512827e-16, 0.0, 0.0); \
    p = fma(p, w, SAM_J1_SEL(0.0, -4.985528380459344e-16, 3.7749320024389593e-16, 0.0, 0.0)); \
    p = fma(p, w, SAM_J1_SEL(0.0, -4.620452642694359e-16, -1.4543114353749935e-13, 0.0, 0.0)); \
    p = fma(p, w, SAM_J1_SEL(0.0, 1.4857739578460684e-13, -5.530674253081099e-14, 0.0, 0.0)); \
    p = fma(p, w, SAM_J1_SEL(-1.4452441443131157e-12, 1.0820822762771697e-13, 3.2351861713992395e-11, 0.0, 0.0)); \
    p = fma(p, w, SAM_J1_SEL(2.601959515046924e-11, -3.323645931584483e-11, -5.993407210051976e-14, 0.0, 0.0)); \
    p = fma(p, w, SAM_J1_SEL(2.802180747276907e-10, -1.7498578515323218e-11, -5.374305504291201e-09, 0.0, -381.50222408965953)); \
    p = fma(p, w, SAM_J1_SEL(-4.4491950190761605e-09, 5.566750999861425e-09, 1.9592721317998253e-09, -16.650717699223307, -1.9958049649578682)); \
    p = fma(p, w, SAM_J1_SEL(-3.9333928716607605e-08, 1.8372423998956471e-09, 6.333857911491498e-07, -1.5182466896291889, 21.693900337498697)); \
    p = fma(p, w, SAM_J1_SEL(5.403062167213952e-07, -6.647394096380015e-07, -4.409090926708715e-07, 2.4765124776520495, -2.8099488256217637)); \
    p = fma(p, w, SAM_J1_SEL(3.7891621189766807e-06, -9.487550367169705e-08, -4.914220994598901e-05, -0.8001635573970287, -1.342692633741042)); \
    p = fma(p, w, SAM_J1_SEL(-4.394234198548893e-05, 5.2730714981338246e-05, 4.7902110363783043e-05, -0.05253860579164713, 0.5101808943874966)); \
    p = fma(p, w, SAM_J1_SEL(-0.0002284533209768204, -1.4957917333048445e-06, 0.0022295065279607806, 0.19253130704615176, 0.11594025776325982)); \
    p = fma(p, w, SAM_J1_SEL(0.0021612137999043454, -0.002490500271862594, -0.0025732147931245794, -0.08084651808243418, -0.13472168454319147)); \
    p = fma(p, w, SAM_J1_SEL(0.007363658579234247, 0.0004155475447138859, -0.04760016896355036, -0.04505420359460063, -0.01762256878316661)); \
    p = fma(p, w, SAM_J1_SEL(-0.0539650753175066, 0.057654931601690995, 0.05327215911799911, 0.11026121597042873, 0.11635210817544757)); \
    p = fma(p, w, SAM_J1_SEL(-0.08943199639953407, -0.013001295522760798, 0.28376249810621745, 0.021523833751794057, 0.007306736168242379)); \
    p = fma(p, w, SAM_J1_SEL(0.4656581362331496, -0.414504406632081, -0.15384130140997185, 1.001019253001245, 1.00011430402634));
/* END GENERATED J1 */
/* BEGIN GENERATED J1Q (tools/make_sa_math_coeffs.py) */
    /* coefficients by piece (zero above a piece's own degree); one Horner chain of degree 11
       piece 0: Q1, 1/x = c + w, c = 0.09375, x in [8.0, 16.0]: degree 10, error 2^-58.9
       piece 1: Q1, 1/x = c + w, c = 0.03125, x in [16.0, inf]: degree 11, error 2^-59.2 */
#define SAM_J1Q_C0 0.09375
#define SAM_J1Q_C1 0.03125
#define SAM_J1Q_HORNER(p, w) \
    p = SAM_J1Q_SEL(0.0, 129.5556070236025); \
    p = fma(p, w, SAM_J1Q_SEL(18.207247151362644, -88.26825631223605)); \
    p = fma(p, w, SAM_J1Q_SEL(-7.60566816196288, 5.058073032491647)); \
    p = fma(p, w, SAM_J1Q_SEL(0.9748768224882792, 5.237459440476077)); \
    p = fma(p, w, SAM_J1Q_SEL(0.5927003164550141, -1.1985438137117657)); \
    p = fma(p, w, SAM_J1Q_SEL(-0.41513460767008337, -0.373671021282917)); \
    p = fma(p, w, SAM_J1Q_SEL(0.06676583793624351, 0.23972891493862133)); \
    p = fma(p, w, SAM_J1Q_SEL(0.08944449595843504, 0.04133888999511256)); \
    p = fma(p, w, SAM_J1Q_SEL(-0.08238593901767037, -0.09989285054109544)); \
    p = fma(p, w, SAM_J1Q_SEL(-0.026806199725188082, -0.009529547503748069)); \
    p = fma(p, w, SAM_J1Q_SEL(0.37239526774274617, 0.37470090339897993)); \
    p = fma(p, w, SAM_J1Q_SEL(0.03507365662484547, 0.01171562897131084));
/* END GENERATED J1Q */

SA_FN double sam_j0(double x, double sn, double cs)
{
    const int k1 = x >= SAM_J0_B1, k2 = x >= SAM_J0_B2, k3 = x >= SAM_J0_B3, k4 = x >= SAM_J0_B4, kq = k4;
    const double t = 1.0 / x;
    const double w = k3 ? t - (k4 ? SAM_J0_C4 : SAM_J0_C3) : x - (k2 ? SAM_J0_C2 : (k1 ? SAM_J0_C1 : SAM_J0_C0));
    const double wq = t - (kq ? SAM_J0Q_C1 : SAM_J0Q_C0);
    double p, q;
    SAM_J0_HORNER(p, w);
    SAM_J0Q_HORNER(q, wq);
    const double osc = (SAM_BSQ2OPI / sqrt(x)) * fma(p, cs, -(q * sn));
    const double u = (x - SAM_J0_Z_HI) - SAM_J0_Z_LO;
    return k3 ? osc : ((k1 && !k2) ? u * p : p);
}

SA_FN double sam_j1(double x, double sn, double cs)
{
    const int k1 = x >= SAM_J1_B1, k2 = x >= SAM_J1_B2, k3 = x >= SAM_J1_B3, k4 = x >= SAM_J1_B4, kq = k4;
    const double t = 1.0 / x;
    const double w = k3 ? t - (k4 ? SAM_J1_C4 : SAM_J1_C3) : x - (k2 ? SAM_J1_C2 : (k1 ? SAM_J1_C1 : SAM_J1_C0));
    const double wq = t - (kq ? SAM_J1Q_C1 : SAM_J1Q_C0);
    double p, q;
    SAM_J1_HORNER(p, w);
    SAM_J1Q_HORNER(q, wq);
    /* chi_1 = chi_0 - pi/2: cos chi_1 = sin chi_0, sin chi_1 = -cos chi_0 */
    const double osc = (SAM_BSQ2OPI / sqrt(x)) * fma(p, sn, q * cs);
    const double u = (x - SAM_J1_Z_HI) - SAM_J1_Z_LO;
    return k3 ? osc : (k1 ? (k2 ? p : u * p) : x * p);
}

/* ---- Y0, Y1 (x > 0 finite, x <= 2^50) ---- */
#define SAM_Y0_B1 0.5            /* below: the logarithmic form */
#define SAM_Y0_B2 1.25
#define SAM_Y0_B3 2.5
#define SAM_Y0_B4 5.0
#define SAM_Y0_B5 8.0            /* from here on: P, Q in 1/x */
#define SAM_Y0_B6 16.0
#define SAM_Y1_B1 0.5
#define SAM_Y1_B2 1.25
#define SAM_Y1_B3 2.5
#define SAM_Y1_B4 5.0
#define SAM_Y1_B5 8.0
#define SAM_Y1_B6 16.0
#define SAM_Y0_SEL(c0, c1, c2, c3, c4, c5) (m5 ? (m6 ? (c5) : (c4)) : (m3 ? (m4 ? (c3) : (c2)) : (m2 ? (c1) : (c0))))
#define SAM_Y1_SEL(c0, c1, c2, c3, c4, c5) SAM_Y0_SEL(c0, c1, c2, c3, c4, c5)
/* BEGIN GENERATED Y0S (tools/make_sa_math_coeffs.py) */
    /* A = (2/pi) J0(x), z = x^2 in [0, 0.25]: degree 6, error 2^-53.6 */
#define SAM_Y0A_POLY(p, z) \
    p = 2.984805684050597e-10; \
    p = fma(p, z, -4.3173082587246796e-08); \
    p = fma(p, z, 4.317354063847922e-06); \
    p = fma(p, z, -0.00027631066508325614); \
    p = fma(p, z, 0.009947183943243173); \
    p = fma(p, z, -0.15915494309189532); \
    p = fma(p, z, 0.6366197723675814);
    /* B = Y0(x) - (2/pi) ln x J0(x), z = x^2 in [0, 0.25]: degree 6, error 2^-52.0 */
#define SAM_Y0B_POLY(p, z) \
    p = -7.656902305666093e-10; \
    p = fma(p, z, 1.0358351761228441e-07); \
    p = fma(p, z, -9.495004993465437e-06); \
    p = fma(p, z, 0.0005386026668431298); \
    p = fma(p, z, -0.016073968025937652); \
    p = fma(p, z, 0.17760601686906713); \
    p = fma(p, z, -0.07380429510868723);
/* END GENERATED Y0S */
/* BEGIN GENERATED Y1S (tools/make_sa_math_coeffs.py) */
    /* A = (2/pi) J1(x)/x, z = x^2 in [0, 0.25]: degree 6, error 2^-53.8 */
#define SAM_Y1A_POLY(p, z) \
    p = 2.1331947173079622e-11; \
    p = fma(p, z, -3.5977664325225833e-09); \
    p = fma(p, z, 4.317354093150526e-07); \
    p = fma(p, z, -3.4538833135834356e-05); \
    p = fma(p, z, 0.0016578639905405585); \
    p = fma(p, z, -0.039788735772973836); \
    p = fma(p, z, 0.3183098861837907);
    /* B = (Y1(x) + (2/pi)/x - (2/pi) ln x J1(x))/x, z = x^2 in [0, 0.25]: degree 6, error 2^-54.4 */
#define SAM_Y1B_POLY(p, z) \
    p = -5.624886120077875e-11; \
    p = fma(p, z, 8.931800132766896e-09); \
    p = fma(p, z, -9.926740483973846e-07); \
    p = fma(p, z, 7.164268749855462e-05); \
    p = fma(p, z, -0.0029553053360797843); \
    p = fma(p, z, 0.05434868816051024); \
    p = fma(p, z, -0.19605709064623894);
/* END GENERATED Y1S */
/* BEGIN GENERATED Y0 (tools/make_sa_math_coeffs.py) */
    /* coefficients by piece (zero above a piece's own degree); one Horner chain of degree 25
       piece 1: Y0(x)/(x - z), z the first zero, x = c + w, c = 0.875, x in [0.5, 1.25]: degree 25, error 2^-54.5
       piece 2: Y0(x), error relative to M0, x = c + w, c = 1.875, x in [1.25, 2.5]: degree 21, error 2^-54.6
       piece 3: Y0(x), error relative to M0, x = c + w, c = 3.75, x in [2.5, 5.0]: degree 21, error 2^-53.1
       piece 4: Y0(x), error relative to M0, x = c + w, c = 6.5, x in [5.0, 8.0]: degree 18, error 2^-53.0
       piece 5: P0, 1/x = c + w, c = 0.09375, x in [8.0, 16.0]: degree 10, error 2^-55.2
       piece 6: P0, 1/x = c + w, c = 0.03125, x in [16.0, inf]: degree 11, error 2^-54.8 */
#define SAM_Y0_C0 0.875
#define SAM_Y0_C1 1.875
#define SAM_Y0_C2 3.75
#define SAM_Y0_C3 6.5
#define SAM_Y0_C4 0.09375
#define SAM_Y0_C5 0.03125
#define SAM_Y0_HORNER(p, w) \
    p = SAM_Y0_SEL(-2.5415634845521824, 0.0, 0.0, 0.0, 0.0, 0.0); \
    p = fma(p, w, SAM_Y0_SEL(2.305085475923861, 0.0, 0.0, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y0_SEL(0.22971058448887213, 0.0, 0.0, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y0_SEL(-0.20299547900318188, 0.0, 0.0, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y0_SEL(-0.7601438843657594, 9.990793999656036e-08, 4.706429945737985e-14, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y0_SEL(0.6941635491870153, -1.9611892655494685e-07, -1.8454386761775102e-13, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y0_SEL(-0.4140760351087957, 1.7118190816640189e-07, 3.206046361870988e-13, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y0_SEL(0.3819338340438836, -3.3953308942985636e-07, -1.2689883358595771e-12, -9.866461810712753e-17, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y0_SEL(-0.38685905127538756, 8.747385415304141e-07, 6.537369664467229e-12, 1.1685185653666051e-15, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y0_SEL(0.3582856058770225, -1.7400107080226875e-06, -2.5943129316701678e-11, -3.171790736148387e-15, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y0_SEL(-0.32951963841303156, 3.3694220722787733e-06, 1.0021539493092824e-10, -1.256156564981892e-13, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y0_SEL(0.3074971383630413, -6.758848201790665e-06, -3.987567426266739e-10, -1.9909994364525838e-13, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y0_SEL(-0.2884526898418979, 1.3655831740871157e-05, 1.5772967016549412e-09, 3.4523561381056215e-11, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y0_SEL(0.27171714926188817, -2.7667989442288076e-05, -6.683668910020717e-09, -1.474720675753004e-11, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y0_SEL(-0.25743446629973454, 5.640134475136602e-05, 3.1362177260579654e-08, -5.503125696145191e-09, 0.0, 345.45934959314604)); \
    p = fma(p, w, SAM_Y0_SEL(0.24557801062071674, -0.00011587331836118684, -7.78735680397302e-08, 2.8885508562774317e-09, 14.271990554839244, 2.932282931531467)); \
    p = fma(p, w, SAM_Y0_SEL(-0.23615961406696206, 0.0002396317229894804, -1.948125237635723e-07, 6.597557736801366e-07, 1.589041959221853, -19.43272387527625)); \
    p = fma(p, w, SAM_Y0_SEL(0.22930368941322696, -0.000494757605910207, -4.418996919897117e-06, -6.425343195455173e-07, -2.190031150713484, 2.4046934361387464)); \
    p = fma(p, w, SAM_Y0_SEL(-0.2252735073855233, 0.0010712054246826606, 5.8633540038817416e-05, -5.095354687002516e-05, 0.6648371739199596, 1.177166184524856)); \
    p = fma(p, w, SAM_Y0_SEL(0.224535506886768, -0.0026943057938775203, 0.00011553940993827711, 6.355454993763605e-05, 0.05811636073147282, -0.4261210687563326)); \
    p = fma(p, w, SAM_Y0_SEL(-0.2283506438963659, 0.004512301902447157, -0.0023783269289142832, 0.002317501714361672, -0.15809607600117354, -0.09772588202361436)); \
    p = fma(p, w, SAM_Y0_SEL(0.2390451175963388, 0.004177015310294184, -0.004475475330594969, -0.003441406645865909, 0.0592936228873087, 0.1041510888841786)); \
    p = fma(p, w, SAM_Y0_SEL(-0.24312447787399188, 0.030915249749415577, 0.06324302209797818, -0.04796153689875436, 0.03449081277031494, 0.013679356117534496)); \
    p = fma(p, w, SAM_Y0_SEL(0.23362165067049984, -0.2940096595864715, 0.012820792090682381, 0.06553727330877768, -0.06496834811470363, -0.06966339443031938)); \
    p = fma(p, w, SAM_Y0_SEL(-0.5005131848545287, 0.1790480194971548, -0.4158687793452271, 0.27409127395927546, -0.012836219732564122, -0.004380941795461027)); \
    p = fma(p, w, SAM_Y0_SEL(0.8886397260567597, 0.4925270421077948, 0.0852567569773627, -0.17324243491898234, 0.9993903253726394, 0.9999314418780413));
/* END GENERATED Y0 */
/* BEGIN GENERATED Y1 (tools/make_sa_math_coeffs.py) */
    /* coefficients by piece (zero above a piece's own degree); one Horner chain of degree 27
       piece 1: Y1(x), x = c + w, c = 0.875, x in [0.5, 1.25]: degree 27, error 2^-54.2
       piece 2: Y1(x)/(x - z), z the first zero, x = c + w, c = 1.875, x in [1.25, 2.5]: degree 22, error 2^-54.7
       piece 3: Y1(x), error relative to M1, x = c + w, c = 3.75, x in [2.5, 5.0]: degree 22, error 2^-54.4
       piece 4: Y1(x), error relative to M1, x = c + w, c = 6.5, x in [5.0, 8.0]: degree 18, error 2^-53.5
       piece 5: P1, 1/x = c + w, c = 0.09375, x in [8.0, 16.0]: degree 10, error 2^-55.4
       piece 6: P1, 1/x = c + w, c = 0.03125, x in [16.0, inf]: degree 11, error 2^-53.2 */
#define SAM_Y1_C0 0.875
#define SAM_Y1_C1 1.875
#define SAM_Y1_C2 3.75
#define SAM_Y1_C3 6.5
#define SAM_Y1_C4 0.09375
#define SAM_Y1_C5 0.03125
#define SAM_Y1_HORNER(p, w) \
    p = SAM_Y1_SEL(106.84839384901414, 0.0, 0.0, 0.0, 0.0, 0.0); \
    p = fma(p, w, SAM_Y1_SEL(-93.48927333311288, 0.0, 0.0, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y1_SEL(-23.378768453540406, 0.0, 0.0, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y1_SEL(20.456331745052335, 0.0, 0.0, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y1_SEL(28.32196411944001, 0.0, 0.0, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y1_SEL(-24.78042556384509, 2.96089293111349e-07, -7.676146779515513e-14, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y1_SEL(9.721849869909096, -5.550088921771515e-07, 2.8749774463475685e-13, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y1_SEL(-8.505668556934271, 3.7525778448192055e-07, -3.869285118902284e-13, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y1_SEL(9.464948445240447, -7.032325298112181e-07, 1.447578718370853e-12, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y1_SEL(-8.280768433909957, 1.9671928473834514e-06, -8.107448209728903e-12, -2.5145327639974707e-16, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y1_SEL(7.009508318818234, -3.6863105166885596e-06, 3.03238308698362e-11, 1.8225124287306325e-15, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y1_SEL(-6.132171198154619, 6.545486007110176e-06, -1.0735977729462098e-10, -1.7464249398517864e-14, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y1_SEL(5.383587897179546, -1.226214442895937e-05, 4.011644005192276e-10, 5.033003757959704e-14, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y1_SEL(-4.709327607896292, 2.309371911483629e-05, -1.507559367584694e-09, 1.874720829737628e-12, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y1_SEL(4.118129743777751, -4.324515089601759e-05, 5.5984334271301095e-09, 2.788943109839344e-12, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y1_SEL(-3.601772088186136, 8.092639238007284e-05, -2.0501727273153272e-08, -4.4878604890595173e-10, 0.0, 0.0)); \
    p = fma(p, w, SAM_Y1_SEL(3.149789882036109, -0.00015143017955710072, 8.019269327032123e-08, 1.7696347354878942e-10, 0.0, -381.50222408965953)); \
    p = fma(p, w, SAM_Y1_SEL(-2.7539698452310537, 0.00028319132158348957, -3.4498536815455805e-07, 6.053435765947974e-08, -16.650717699223307, -1.9958049649578682)); \
    p = fma(p, w, SAM_Y1_SEL(2.4072170396530534, -0.0005291900983061134, 7.787407423595348e-07, -2.88855052436031e-08, -1.5182466896291889, 21.693900337498697)); \
    p = fma(p, w, SAM_Y1_SEL(-2.1032172663220927, 0.0009882640116430864, 1.7533131010194985e-06, -5.9378019450922486e-06, 2.4765124776520495, -2.8099488256217637)); \
    p = fma(p, w, SAM_Y1_SEL(1.836266194288891, -0.0018383246275097565, 3.5351974006608373e-05, 5.140274554298862e-06, -0.8001635573970287, -1.342692633741042)); \
    p = fma(p, w, SAM_Y1_SEL(-1.601042837656437, 0.003365860188199037, -0.00041043478033026454, 0.00035667482808291866, -0.05253860579164713, 0.5101808943874966)); \
    p = fma(p, w, SAM_Y1_SEL(1.395130994623279, -0.006414155316086171, -0.0006932364594320896, -0.0003813272996251397, 0.19253130704615176, 0.11594025776325982)); \
    p = fma(p, w, SAM_Y1_SEL(-1.2164358990343322, 0.01409957027636944, 0.011891634644575577, -0.011587508571806907, -0.08084651808243418, -0.13472168454319147)); \
    p = fma(p, w, SAM_Y1_SEL(0.9902608438510758, -0.01801945524680411, 0.01790190132236673, 0.013765626583463537, -0.04505420359460063, -0.01762256878316661)); \
    p = fma(p, w, SAM_Y1_SEL(-0.7144144976928237, -0.02251287244893967, -0.18972906629393466, 0.143884610696263, 0.11026121597042873, 0.11635210817544757)); \
    p = fma(p, w, SAM_Y1_SEL(1.009706332762236, -0.09999807583171608, -0.025641584181364505, -0.13107454661755533, 0.021523833751794057, 0.007306736168242379)); \
    p = fma(p, w, SAM_Y1_SEL(-0.897937742614081, 0.5558058064239648, 0.4158687793452271, -0.27409127395927546, 1.001019253001245, 1.00011430402634));
/* END GENERATED Y1 */

SA_FN double sam_y0(double x, double sn, double cs)
{
    const int m1 = x >= SAM_Y0_B1, m2 = x >= SAM_Y0_B2, m3 = x >= SAM_Y0_B3, m4 = x >= SAM_Y0_B4, m5 = x >= SAM_Y0_B5,
              m6 = x >= SAM_Y0_B6, kq = m6;
    const double t = 1.0 / x;
    const double w = m5 ? t - (m6 ? SAM_Y0_C5 : SAM_Y0_C4)
                        : x - (m3 ? (m4 ? SAM_Y0_C3 : SAM_Y0_C2) : (m2 ? SAM_Y0_C1 : SAM_Y0_C0));
    const double wq = t - (kq ? SAM_J0Q_C1 : SAM_J0Q_C0);
    double p, q, a, b;
    SAM_Y0_HORNER(p, w);
    SAM_J0Q_HORNER(q, wq);
    const double z = x * x;
    SAM_Y0A_POLY(a, z);
    SAM_Y0B_POLY(b, z);
    const double small = fma(sa_log(x), a, b);
    const double osc = (SAM_BSQ2OPI / sqrt(x)) * fma(p, sn, q * cs);
    const double u = (x - SAM_Y0_Z_HI) - SAM_Y0_Z_LO;
    return m5 ? osc : (m1 ? (m2 ? p : u * p) : small);
}

SA_FN double sam_y1(double x, double sn, double cs)
{
    const int m1 = x >= SAM_Y1_B1, m2 = x >= SAM_Y1_B2, m3 = x >= SAM_Y1_B3, m4 = x >= SAM_Y1_B4, m5 = x >= SAM_Y1_B5,
              m6 = x >= SAM_Y1_B6, kq = m6;
    const double t = 1.0 / x;
    const double w = m5 ? t - (m6 ? SAM_Y1_C5 : SAM_Y1_C4)
                        : x - (m3 ? (m4 ? SAM_Y1_C3 : SAM_Y1_C2) : (m2 ? SAM_Y1_C1 : SAM_Y1_C0));
    const double wq = t - (kq ? SAM_J1Q_C1 : SAM_J1Q_C0);
    double p, q, a, b;
    SAM_Y1_HORNER(p, w);
    SAM_J1Q_HORNER(q, wq);
    const double z = x * x;
    SAM_Y1A_POLY(a, z);
    SAM_Y1B_POLY(b, z);
    const double small = fma(x, fma(sa_log(x), a, b), -(SAM_B2OPI / x));
    const double osc = (SAM_BSQ2OPI / sqrt(x)) * fma(q, sn, -(p * cs));
    const double u = (x - SAM_Y1_Z_HI) - SAM_Y1_Z_LO;
    return m5 ? osc : (m1 ? ((m2 && !m3) ? u * p : p) : small);
}

/* ---- I0, I1 (a >= 0 finite): the value without the factor exp(32) of a > 700 (sam_bessel_far applies it) ---- */
#define SAM_I0_B1 8.0            /* from here on: sqrt(a) exp(-a) I(a) in 1/a */
#define SAM_I0_B2 16.0
#define SAM_I1_B1 8.0
#define SAM_I1_B2 16.0
#define SAM_I_FAR 700.0
#define SAM_I0_SEL(c0, c1, c2) (k1 ? (k2 ? (c2) : (c1)) : (c0))
#define SAM_I1_SEL(c0, c1, c2) SAM_I0_SEL(c0, c1, c2)
/* BEGIN GENERATED I0 (tools/make_sa_math_coeffs.py) */
    /* coefficients by piece (zero above a piece's own degree); one Horner chain of degree 16
       piece 0: I0(x), w = x^2 in [0, 64.0]: degree 16, error 2^-55.0
       piece 1: sqrt(x) exp(-x) I0(x), 1/x = c + w, c = 0.09375, x in [8.0, 16.0]: degree 15, error 2^-55.0
       piece 2: sqrt(x) exp(-x) I0(x), 1/x = c + w, c = 0.03125, x in [16.0, inf]: degree 13, error 2^-54.0 */
#define SAM_I0_C1 0.09375
#define SAM_I0_C2 0.03125
#define SAM_I0_HORNER(p, w) \
    p = SAM_I0_SEL(8.487698345602824e-37, 0.0, 0.0); \
    p = fma(p, w, SAM_I0_SEL(4.601357767863732e-34, -39001226.62174583, 0.0)); \
    p = fma(p, w, SAM_I0_SEL(5.0327117729737235e-31, 299091219.1546398, 0.0)); \
    p = fma(p, w, SAM_I0_SEL(3.829411247002327e-28, -11478920.864066813, 642133.8253173741)); \
    p = fma(p, w, SAM_I0_SEL(2.5987841051325663e-25, -3830237.067523196, 57017.21033429871)); \
    p = fma(p, w, SAM_I0_SEL(1.4962822964042478e-22, 196893.86062155015, 3017.3924469705867)); \
    p = fma(p, w, SAM_I0_SEL(7.242279005317181e-20, 41018.00291002344, 351.4547653692492)); \
    p = fma(p, w, SAM_I0_SEL(2.896902788810415e-17, -1527.6228258111205, 54.60389779479808)); \
    p = fma(p, w, SAM_I0_SEL(9.385967122158306e-15, -510.2180816058227, 9.3174520788131)); \
    p = fma(p, w, SAM_I0_SEL(2.4028075474081917e-12, -19.106923623610374, 1.9153032908443806)); \
    p = fma(p, w, SAM_I0_SEL(4.709502797312111e-10, 3.7681769867209574, 0.4837888129539841)); \
    p = fma(p, w, SAM_I0_SEL(6.781684027758202e-08, 0.8871473839816496, 0.15333707955587259)); \
    p = fma(p, w, SAM_I0_SEL(6.781684027778812e-06, 0.18367424976679014, 0.06319051473429002)); \
    p = fma(p, w, SAM_I0_SEL(0.00043402777777777445, 0.06223896810801007, 0.035864386211409055)); \
    p = fma(p, w, SAM_I0_SEL(0.015625000000000007, 0.03984538506608847, 0.031083533790742073)); \
    p = fma(p, w, SAM_I0_SEL(0.25, 0.05609571928059161, 0.05171249281224818)); \
    p = fma(p, w, SAM_I0_SEL(1.0, 0.4038923361468227, 0.40052897918718267));
/* END GENERATED I0 */
/* BEGIN GENERATED I1 (tools/make_sa_math_coeffs.py) */
    /* coefficients by piece (zero above a piece's own degree); one Horner chain of degree 15
       piece 0: I1(x)/x, w = x^2 in [0, 64.0]: degree 15, error 2^-54.1
       piece 1: sqrt(x) exp(-x) I1(x), 1/x = c + w, c = 0.09375, x in [8.0, 16.0]: degree 15, error 2^-53.7
       piece 2: sqrt(x) exp(-x) I1(x), 1/x = c + w, c = 0.03125, x in [16.0, inf]: degree 13, error 2^-54.4 */
#define SAM_I1_C1 0.09375
#define SAM_I1_C2 0.03125
#define SAM_I1_HORNER(p, w) \
    p = SAM_I1_SEL(2.716505589516919e-35, -103499870.08601841, 0.0); \
    p = fma(p, w, SAM_I1_SEL(1.3808181584914298e-32, -307503188.55894655, 0.0)); \
    p = fma(p, w, SAM_I1_SEL(1.408926251589232e-29, 13857606.834850976, -679626.9189907534)); \
    p = fma(p, w, SAM_I1_SEL(9.956969230500738e-27, 3915318.5236446597, -60412.09027991521)); \
    p = fma(p, w, SAM_I1_SEL(6.2370206832638684e-24, -225698.7899247897, -3232.126457825541)); \
    p = fma(p, w, SAM_I1_SEL(3.2918259018287706e-21, -42215.00576928186, -381.46231251566707)); \
    p = fma(p, w, SAM_I1_SEL(1.448455537254395e-18, 1840.1655323622101, -59.85717974621754)); \
    p = fma(p, w, SAM_I1_SEL(5.214425120919993e-16, 543.0908813914018, -10.361781647486964)); \
    p = fma(p, w, SAM_I1_SEL(1.5017547367976848e-13, 18.25305029669156, -2.1698460277587324)); \
    p = fma(p, w, SAM_I1_SEL(3.3639305668982475e-11, -4.351419489984279, -0.5616271846425028)); \
    p = fma(p, w, SAM_I1_SEL(5.651403356704746e-09, -1.0113858300773042, -0.18416870308662076)); \
    p = fma(p, w, SAM_I1_SEL(6.781684027764357e-07, -0.21951352877314737, -0.07986853554712466)); \
    p = fma(p, w, SAM_I1_SEL(5.42534722222271e-05, -0.08175866351560297, -0.04937623965876751)); \
    p = fma(p, w, SAM_I1_SEL(0.0026041666666666574, -0.06274903222128317, -0.05096139881081227)); \
    p = fma(p, w, SAM_I1_SEL(0.06250000000000001, -0.159698290158575, -0.15265274530923523)); \
    p = fma(p, w, SAM_I1_SEL(0.5, 0.38446685410720083, 0.394220213406121));
/* END GENERATED I1 */

/* exp(a) / sqrt(a) without the factor exp(32) of a > SAM_I_FAR */
SA_FN double sam_bessel_grow(double a)
{
    return sa_exp((a > SAM_I_FAR) ? a - 32.0 : a) / sqrt(a);
}

SA_FN double sam_bessel_far(double v, double a)
{
    return (a > SAM_I_FAR) ? fma(v, SAM_BE32_LO, v * SAM_BE32_HI) : v;
}

SA_FN double sam_i0(double a)
{
    const int k1 = a >= SAM_I0_B1, k2 = a >= SAM_I0_B2;
    const double w = k1 ? 1.0 / a - (k2 ? SAM_I0_C2 : SAM_I0_C1) : a * a;
    double p;
    SAM_I0_HORNER(p, w);
    return k1 ? p * sam_bessel_grow(a) : p;
}

SA_FN double sam_i1(double a)
{
    const int k1 = a >= SAM_I1_B1, k2 = a >= SAM_I1_B2;
    const double w = k1 ? 1.0 / a - (k2 ? SAM_I1_C2 : SAM_I1_C1) : a * a;
    double p;
    SAM_I1_HORNER(p, w);
    return k1 ? p * sam_bessel_grow(a) : a * p;
}

/* ---- K0, K1 (x > 0 finite): the value below 1, exp(x) K(x) from 1 on ---- */
#define SAM_K0_B1 1.0            /* below: the logarithmic form */
#define SAM_K0_B2 2.0
#define SAM_K0_B3 4.0
#define SAM_K0_B4 8.0
#define SAM_K0_B5 16.0
#define SAM_K1_B1 1.0
#define SAM_K1_B2 2.0
#define SAM_K1_B3 4.0
#define SAM_K1_B4 8.0
#define SAM_K1_B5 16.0
#define SAM_K0_SEL(c0, c1, c2, c3, c4) (k4 ? (k5 ? (c4) : (c3)) : (k3 ? (c2) : (k2 ? (c1) : (c0))))
#define SAM_K1_SEL(c0, c1, c2, c3, c4) SAM_K0_SEL(c0, c1, c2, c3, c4)
/* BEGIN GENERATED K0S (tools/make_sa_math_coeffs.py) */
    /* A = I0(x), z = x^2 in [0, 1.0]: degree 7, error 2^-55.9 */
#define SAM_K0A_POLY(p, z) \
    p = 2.4406278948541674e-12; \
    p = fma(p, z, 4.708886739799705e-10); \
    p = fma(p, z, 6.781689246632508e-08); \
    p = fma(p, z, 6.781684003298254e-06); \
    p = fma(p, z, 0.00043402777778401143); \
    p = fma(p, z, 0.015624999999999221); \
    p = fma(p, z, 0.25000000000000006); \
    p = fma(p, z, 1.0);
    /* B = K0(x) + ln x I0(x), z = x^2 in [0, 1.0]: degree 8, error 2^-55.7 */
#define SAM_K0B_POLY(p, z) \
    p = 2.6984361912313664e-14; \
    p = fma(p, z, 6.507971505261944e-12); \
    p = fma(p, z, 1.208426900211292e-09); \
    p = fma(p, z, 1.627105606146431e-07); \
    p = fma(p, z, 1.4914719299410551e-05); \
    p = fma(p, z, 0.0008460350907081938); \
    p = fma(p, z, 0.025248929932162698); \
    p = fma(p, z, 0.2789828789146031); \
    p = fma(p, z, 0.11593151565841245);
/* END GENERATED K0S */
/* BEGIN GENERATED K1S (tools/make_sa_math_coeffs.py) */
    /* A = I1(x)/x, z = x^2 in [0, 1.0]: degree 7, error 2^-58.1 */
#define SAM_K1A_POLY(p, z) \
    p = 1.522750603604819e-13; \
    p = fma(p, z, 3.363588648332749e-11); \
    p = fma(p, z, 5.6514062526881675e-09); \
    p = fma(p, z, 6.781684014193744e-07); \
    p = fma(p, z, 5.425347222256812e-05); \
    p = fma(p, z, 0.0026041666666666236); \
    p = fma(p, z, 0.0625); \
    p = fma(p, z, 0.5);
    /* B = (K1(x) - 1/x - ln x I1(x))/x, z = x^2 in [0, 1.0]: degree 7, error 2^-54.3 */
#define SAM_K1B_POLY(p, z) \
    p = -4.2224747994537033e-13; \
    p = fma(p, z, -8.870907975584019e-11); \
    p = fma(p, z, -1.403017207152258e-08); \
    p = fma(p, z, -1.5592887662774348e-06); \
    p = fma(p, z, -0.00011253607036730547); \
    p = fma(p, z, -0.004642182766471435); \
    p = fma(p, z, -0.08537071972865079); \
    p = fma(p, z, -0.3079657578292062);
/* END GENERATED K1S */
/* BEGIN GENERATED K0 (tools/make_sa_math_coeffs.py) */
    /* coefficients by piece (zero above a piece's own degree); one Horner chain of degree 15
       piece 1: sqrt(x) exp(x) K0(x), 1/x = c + w, c = 0.75, x in [1.0, 2.0]: degree 15, error 2^-53.2
       piece 2: sqrt(x) exp(x) K0(x), 1/x = c + w, c = 0.375, x in [2.0, 4.0]: degree 13, error 2^-55.9
       piece 3: sqrt(x) exp(x) K0(x), 1/x = c + w, c = 0.1875, x in [4.0, 8.0]: degree 11, error 2^-54.0
       piece 4: sqrt(x) exp(x) K0(x), 1/x = c + w, c = 0.09375, x in [8.0, 16.0]: degree 10, error 2^-55.7
       piece 5: sqrt(x) exp(x) K0(x), 1/x = c + w, c = 0.03125, x in [16.0, inf]: degree 10, error 2^-55.0 */
#define SAM_K0_C0 0.75
#define SAM_K0_C1 0.375
#define SAM_K0_C2 0.1875
#define SAM_K0_C3 0.09375
#define SAM_K0_C4 0.03125
#define SAM_K0_HORNER(p, w) \
    p = SAM_K0_SEL(-0.00011492470037571309, 0.0, 0.0, 0.0, 0.0); \
    p = fma(p, w, SAM_K0_SEL(0.00013787788061238996, 0.0, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_K0_SEL(-0.00013975604692995249, -0.03668661969856681, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_K0_SEL(0.0001757210823030448, 0.027528408909944253, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_K0_SEL(-0.00022922683624194824, -0.019294708165983523, -0.7105091362976773, 0.0, 0.0)); \
    p = fma(p, w, SAM_K0_SEL(0.000303089428681894, 0.015565444188473712, 0.3733910744639399, 3.6330543117037175, 32.41117466109962)); \
    p = fma(p, w, SAM_K0_SEL(-0.0004135906368391367, -0.013125394979068308, -0.19838373853290314, -1.4529188412316525, -9.223013110546216)); \
    p = fma(p, w, SAM_K0_SEL(0.0005862788747429208, 0.011569130794557231, 0.11721570440264137, 0.6164782331695858, 2.8005818063852517)); \
    p = fma(p, w, SAM_K0_SEL(-0.0008695663692846125, -0.010799973379307774, -0.0744710393065173, -0.2908245494381781, -0.9847912484759725)); \
    p = fma(p, w, SAM_K0_SEL(0.001363766899594035, 0.0108164909112579, 0.051599661373996276, 0.15244082347484691, 0.3942081765490681)); \
    p = fma(p, w, SAM_K0_SEL(-0.0022963671774693865, -0.011836558949526593, -0.039862046765630946, -0.09093886571542745, -0.18436553840970166)); \
    p = fma(p, w, SAM_K0_SEL(0.004250067927479478, 0.014551554773086423, 0.03545213806946566, 0.06397383116658106, 0.10470004371058057)); \
    p = fma(p, w, SAM_K0_SEL(-0.008993309628035422, -0.02104006312428899, -0.038228729227230356, -0.05614096304369905, -0.07662853120613627)); \
    p = fma(p, w, SAM_K0_SEL(0.023469052677277173, 0.038992808987245796, 0.05495007451195605, 0.06797382614505247, 0.08026364520969505)); \
    p = fma(p, w, SAM_K0_SEL(-0.09081693634584095, -0.11342093762206781, -0.13073846099740463, -0.1421844958181737, -0.15140955415155924)); \
    p = fma(p, w, SAM_K0_SEL(1.1658263717940323, 1.2037634037320846, 1.226560671018869, 1.239334928758195, 1.2485017620221532));
/* END GENERATED K0 */
/* BEGIN GENERATED K1 (tools/make_sa_math_coeffs.py) */
    /* coefficients by piece (zero above a piece's own degree); one Horner chain of degree 15
       piece 1: sqrt(x) exp(x) K1(x), 1/x = c + w, c = 0.75, x in [1.0, 2.0]: degree 15, error 2^-55.0
       piece 2: sqrt(x) exp(x) K1(x), 1/x = c + w, c = 0.375, x in [2.0, 4.0]: degree 13, error 2^-55.5
       piece 3: sqrt(x) exp(x) K1(x), 1/x = c + w, c = 0.1875, x in [4.0, 8.0]: degree 11, error 2^-54.3
       piece 4: sqrt(x) exp(x) K1(x), 1/x = c + w, c = 0.09375, x in [8.0, 16.0]: degree 10, error 2^-54.0
       piece 5: sqrt(x) exp(x) K1(x), 1/x = c + w, c = 0.03125, x in [16.0, inf]: degree 10, error 2^-53.5 */
#define SAM_K1_C0 0.75
#define SAM_K1_C1 0.375
#define SAM_K1_C2 0.1875
#define SAM_K1_C3 0.09375
#define SAM_K1_C4 0.03125
#define SAM_K1_HORNER(p, w) \
    p = SAM_K1_SEL(0.00013851722633723867, 0.0, 0.0, 0.0, 0.0); \
    p = fma(p, w, SAM_K1_SEL(-0.00016747338347037764, 0.0, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_K1_SEL(0.0001718175049181871, 0.04304979164668564, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_K1_SEL(-0.0002182499789751808, -0.03257957608819501, 0.0, 0.0, 0.0)); \
    p = fma(p, w, SAM_K1_SEL(0.00028792415054855334, 0.023105552009316084, 0.8221664997147149, 0.0, 0.0)); \
    p = fma(p, w, SAM_K1_SEL(-0.00038596120560922755, -0.01886070182090898, -0.4366077332907128, -4.1530000249546575, -36.28707352747118)); \
    p = fma(p, w, SAM_K1_SEL(0.0005353480105635541, 0.016127591106627863, 0.23513649832818226, 1.6805846936012463, 10.442944581754299)); \
    p = fma(p, w, SAM_K1_SEL(-0.0007740313419111708, -0.014462627727587586, -0.1411174978565891, -0.7239045582543482, -3.218440215985142)); \
    p = fma(p, w, SAM_K1_SEL(0.0011766564711904127, 0.013796920513612044, 0.09144636745008126, 0.34796369764220053, 1.152388537887252)); \
    p = fma(p, w, SAM_K1_SEL(-0.0019048559701035823, -0.014213487172868834, -0.0650323334037383, -0.18697547355398705, -0.4725495484628621)); \
    p = fma(p, w, SAM_K1_SEL(0.003347760053267225, 0.016165403794679102, 0.052078442008444435, 0.11546433235299744, 0.22859986387707268)); \
    p = fma(p, w, SAM_K1_SEL(-0.006590865416667872, -0.021028165873163234, -0.048853569129848756, -0.0855367291621869, -0.13658908792927632)); \
    p = fma(p, w, SAM_K1_SEL(0.015399590466387725, 0.03334205503316997, 0.0575406502421621, 0.08183178296112534, 0.10887439590705673)); \
    p = fma(p, w, SAM_K1_SEL(-0.0487245090529894, -0.07421450891040955, -0.0988254279004978, -0.11810673897631828, -0.1357881085601284)); \
    p = fma(p, w, SAM_K1_SEL(0.3482171781646587, 0.39309536275095125, 0.4251218980336152, 0.44535332976624553, 0.46116922037347957)); \
    p = fma(p, w, SAM_K1_SEL(1.551926734522259, 1.4135192225787472, 1.336954459907448, 1.2961790851234585, 1.2678617411610231));
/* END GENERATED K1 */

SA_FN double sam_k0(double x)
{
    const int k1 = x >= SAM_K0_B1, k2 = x >= SAM_K0_B2, k3 = x >= SAM_K0_B3, k4 = x >= SAM_K0_B4, k5 = x >= SAM_K0_B5;
    const double w = 1.0 / x - (k4 ? (k5 ? SAM_K0_C4 : SAM_K0_C3) : (k3 ? SAM_K0_C2 : (k2 ? SAM_K0_C1 : SAM_K0_C0)));
    double p, a, b;
    SAM_K0_HORNER(p, w);
    const double z = x * x;
    SAM_K0A_POLY(a, z);
    SAM_K0B_POLY(b, z);
    return k1 ? p / sqrt(x) : fma(-sa_log(x), a, b);
}

SA_FN double sam_k1(double x)
{
    const int k1 = x >= SAM_K1_B1, k2 = x >= SAM_K1_B2, k3 = x >= SAM_K1_B3, k4 = x >= SAM_K1_B4, k5 = x >= SAM_K1_B5;
    const double t = 1.0 / x;
    const double w = t - (k4 ? (k5 ? SAM_K1_C4 : SAM_K1_C3) : (k3 ? SAM_K1_C2 : (k2 ? SAM_K1_C1 : SAM_K1_C0)));
    double p, a, b;
    SAM_K1_HORNER(p, w);
    const double z = x * x;
    SAM_K1A_POLY(a, z);
    SAM_K1B_POLY(b, z);
    return k1 ? p / sqrt(x) : fma(x, fma(sa_log(x), a, b), t);
}

/* ---- orders >= 2 ---- */
#define SAM_JN_B1 1.0            /* |x| below: the power series (J and I); J: the downward recurrence up to |x| = n */
#define SAM_JN_EXTRA 14          /* J: the downward recurrence starts at order 3n + 14 (J of that order is below 2^-56 for |x| < n) */
#define SAM_IN_B1 1.0
#define SAM_IN_B2 50.0           /* I: from here on Hankel's asymptotic series */
#define SAM_IN_START 48          /* I: the downward recurrence starts at this order */
#define SAM_IN_TERMS 18
#define SAM_BESSEL_SERIES 10

/* (a/2)^n / n! * sum_k (sg z)^k / (k! (n + 1)...(n + k)), z = a^2/4, 0 <= a < 1, n >= 2; sg = -1: J_n, +1: I_n */
SA_FN double sam_bessel_series(int n, double a, double sg)
{
    const double h = 0.5 * a;
    const double z = sg * (h * h);
    double s = 1.0, pw = h, fact = 1.0;
    for (int k = SAM_BESSEL_SERIES; k >= 1; k--)
        s = fma(z / (double)(k * (n + k)), s, 1.0);
    for (int k = 2; k <= n; k++) {
        pw = pw * h;
        fact = fact * (double)k;
    }
    return (pw / fact) * s;
}

SAM_BESSEL_FN double sa_bessel_j(int n, double x)
{
    if (!(x == x)) return x;
    const double a = fabs(x);
    const double sign = ((n & 1) && x < 0.0) ? -1.0 : 1.0;
    if (a == SAM_INF) return sign * 0.0;
    if (!(a <= SAM_BESSEL_XMAX)) return SAM_NAN;
    if (a == 0.0) return (n == 0) ? 1.0 : ((n & 1) ? x : 0.0);
    if (n >= 2 && a < (double)n) {
        if (a < SAM_JN_B1) return sign * sam_bessel_series(n, a, -1.0);
        /* y_{k-1} = (2k/a) y_k - y_{k+1} downwards from y_{N+1} = 0, y_N = 1; J_n = y_n / (y_0 + 2 (y_2 + y_4 + ...)) */
        const double tx = 2.0 / a;
        double yp = 0.0, yc = 1.0, sum = 0.0, yn = 0.0;
        for (int k = 3 * n + SAM_JN_EXTRA; k >= 1; k--) {
            yn = (k == n) ? yc : yn;
            sum = (k & 1) ? sum : sum + yc;
            const double ym = fma((double)k * tx, yc, -yp);
            yp = yc;
            yc = ym;
        }
        return sign * (yn / fma(2.0, sum, yc));
    }
    double sn, cs;
    sam_bessel_phase(a, &sn, &cs);
    double prev = sam_j0(a, sn, cs), cur = sam_j1(a, sn, cs);
    if (n == 0) return prev;
    if (n >= 2) {
        const double tx = 2.0 / a;
        for (int k = 1; k < n; k++) {
            const double next = fma((double)k * tx, cur, -prev);
            prev = cur;
            cur = next;
        }
    }
    return sign * cur;
}

SAM_BESSEL_FN double sa_bessel_y(int n, double x)
{
    if (!(x == x)) return x;
    if (x < 0.0) return SAM_NAN;
    if (x == 0.0) return -SAM_INF;
    if (x == SAM_INF) return 0.0;
    if (!(x <= SAM_BESSEL_XMAX)) return SAM_NAN;
    double sn, cs;
    sam_bessel_phase(x, &sn, &cs);
    double prev = sam_y0(x, sn, cs), cur = sam_y1(x, sn, cs);
    if (n == 0) return prev;
    if (n >= 2) {
        const double tx = 2.0 / x;
        for (int k = 1; k < n; k++) {
            const double next = fma((double)k * tx, cur, -prev);
            prev = cur;
            cur = next;
        }
        cur = (cur == cur) ? cur : -SAM_INF;                     /* (-inf) - (-inf) of an overflowed recurrence */
    }
    return cur;
}

SAM_BESSEL_FN double sa_bessel_i(int n, double x)
{
    if (!(x == x)) return x;
    const double a = fabs(x);
    const double sign = ((n & 1) && x < 0.0) ? -1.0 : 1.0;
    if (a == SAM_INF) return sign * SAM_INF;
    if (a == 0.0) return (n == 0) ? 1.0 : ((n & 1) ? x : 0.0);
    if (n == 0) return sam_bessel_far(sam_i0(a), a);
    if (n == 1) return sign * sam_bessel_far(sam_i1(a), a);
    if (a < SAM_IN_B1) return sign * sam_bessel_series(n, a, 1.0);
    if (a >= SAM_IN_B2) {
        /* exp(a) / sqrt(2 pi a) (1 - (mu - 1)/(8a) + (mu - 1)(mu - 9)/(2! (8a)^2) - ...), mu = 4 n^2 */
        const double mu = (double)(4 * n * n), e = 0.125 / a;
        double s = 1.0;
        for (int k = SAM_IN_TERMS; k >= 1; k--)
            s = fma(-((mu - (double)((2 * k - 1) * (2 * k - 1))) / (double)k) * e, s, 1.0);
        return sign * sam_bessel_far((s * SAM_BISQ2PI) * sam_bessel_grow(a), a);
    }
    /* y_{k-1} = y_{k+1} + (2k/a) y_k downwards from y_{N+1} = 0, y_N = 1; I_n = I_0 y_n / y_0 */
    const double tx = 2.0 / a;
    double yp = 0.0, yc = 1.0, yn = 0.0;
    for (int k = SAM_IN_START; k >= 1; k--) {
        yn = (k == n) ? yc : yn;
        const double ym = fma((double)k * tx, yc, yp);
        yp = yc;
        yc = ym;
    }
    return sign * ((yn / yc) * sam_i0(a));
}

SAM_BESSEL_FN double sa_bessel_k(int n, double x)
{
    if (!(x == x)) return x;
    if (x < 0.0) return SAM_NAN;
    if (x == 0.0) return SAM_INF;
    if (x == SAM_INF) return 0.0;
    double prev = sam_k0(x), cur = sam_k1(x);
    cur = (n == 0) ? prev : cur;
    if (n >= 2) {
        const double tx = 2.0 / x;
        for (int k = 1; k < n; k++) {
            const double next = fma((double)k * tx, cur, prev);
            prev = cur;
            cur = next;
        }
    }
    return (x >= SAM_K0_B1) ? cur * sa_exp(-x) : cur;
}
#endif /* SA_MATH_BESSEL_H */
