/*
 * pinned_math.h -- the handful of transcendental functions the detection path
 * needs, written once in plain IEEE-754 arithmetic (+ - * / and bit moves only)
 * so that the SAME source gives the SAME bits on the host (gcc, used by the
 * CPU oracle) and on the device (hipcc, gfx950).  Both sides must be compiled
 * with -ffp-contract=off and without fast-math; nothing here may be replaced
 * by a library call.
 *
 * Why it exists: the reference leaves these to the platform libm
 *   - cv::fitEllipseDirect        -> atan2 (double)        (src/objdetect.cpp:68)
 *   - cv::RotatedRect::points     -> sin, cos (double)     (src/core.cpp:268)
 *   - rm::filter_armours          -> atan2 on floats       (src/objdetect.cpp:137)
 *   - rm::utils::ExtendCord       -> atan2/sin/cos floats  (src/core.cpp:335-337)
 * and a GPU has no glibc.  Every double result on this path is narrowed to
 * float before it is used, so a <=1 ulp (double) difference from glibc changes
 * an output bit with probability ~2^-29 per call; tests/test_pinned_math.py
 * measures the agreement with the host libm.
 *
 * Method: classic Cody-Waite reduction by pi/2 (three 33/33/53-bit pieces) and
 * the well-known degree-13/14 minimax kernels on [-pi/4, pi/4]; arctangent by
 * the usual 4-breakpoint reduction + odd/even split degree-11 polynomial in
 * x^2.  Coefficients were re-verified against mpmath (rel. error < 5e-18).
 * Float variants evaluate in double and round once (correctly rounded float
 * results except with probability ~2^-29).
 *
 * pm_tan (rm::DeltaHeight, src/mobility.cpp:48, for device-resident aiming) is the classical kernel
 * tangent behind the same reduction, |error| < 1 ulp (tests/test_pinned_tan.py).
 *
 * pm_hypot (the device tracker's Jacobi rotation) is the one function here that
 * is CORRECTLY ROUNDED, and the one that uses sqrt and the explicit fma besides:
 * see its own comment.
 *
 * "The same bits" is tested directly: tests/leaf/leaf_main.hip evaluates every function of this file in a trivial kernel and in hipcc's host
 * pass, tests/leaf/leaf_host_main.c with gcc, and the three must agree bit for bit (NaNs as a class) over tests/leaf_cases.py
 * (tests/test_leaf_cpu.py, tests/test_gpu_leaf.py).
 *
 * Accuracy against the TRUE value (mpmath at 200 bits, tests/test_leaf_cpu.py; the comparisons with glibc above say nothing about it).
 * Max error measured over that case list, in ulp of the true value, and the bound the test holds it to:
 *     pm_sin 0.79, pm_cos 0.80, pm_tan 0.75 (|x| <= 1e4), pm_acos 0.83                           below 1
 *     pm_atan 0.74, pm_atan2 1.26, pm_log 0.78, pm_exp 1.09                                       at most 2
 *     pm_hypot                                                                                    the correctly rounded value, always
 *     pm_pow, all 2 011 575 pairs (i, gamma) with |g ln x| <= 700: relative error up to           (2.5 |g ln x| + 2) 2^-53, each pair
 *       987 x 2^-53 (at |g ln x| = 600); never more than 0.842 of the pair's own bound            against its own
 *     pm_atan2f, pm_sinf, pm_cosf: no result of 800 000 differs from the correctly rounded float  at most 1 in 2^20; none on integer
 *                                                                                                 pairs in [-64, 64]^2 (contour points)
 * Defined everywhere: no input makes a conversion or a shift undefined (tests/test_leaf_cpu.py runs the list under
 * -fsanitize=undefined,float-cast-overflow); see pm_rem_pio2 for the one edge that needed a rule.
 */
#ifndef RMCV_PINNED_MATH_H
#define RMCV_PINNED_MATH_H

#include <stdint.h>

#if defined(__HIPCC__)
#define PM_FN __host__ __device__ static inline
#else
#define PM_FN static inline
#endif

PM_FN double pm_fabs(double x) { return x < 0 ? -x : (x == 0 ? 0.0 : x); }

PM_FN double pm_hi_word_only(double x)
{
    uint64_t u;
    __builtin_memcpy(&u, &x, 8);
    u &= 0xFFFFFFFF00000000ull;
    __builtin_memcpy(&x, &u, 8);
    return x;
}

/* sin on [-pi/4, pi/4]; y is the tail of x */
PM_FN double pm_ksin(double x, double y, int have_tail)
{
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
                 S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                 S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    double z = x * x;
    double v = z * x;
    double r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    if (!have_tail) return x + v * (S1 + z * r);
    return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}

/* cos on [-pi/4, pi/4]; y is the tail of x */
PM_FN double pm_kcos(double x, double y)
{
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
                 C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                 C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    double ax = pm_fabs(x);
    double z = x * x;
    double r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    if (ax < 0.3) return 1.0 - (0.5 * z - (z * r - x * y));
    {
        double qx = (ax > 0.78125) ? 0.28125 : pm_hi_word_only(ax * 0.25);
        double hz = 0.5 * z - qx;
        double a = 1.0 - qx;
        return a - (hz - (z * r - x * y));
    }
}

/* reduce x to r+t with |r| <= pi/4 (+eps); returns quadrant n mod 4.
 * Accurate for |x| < ~1e5 (n*p1 and n*p2 exact while |n| < 2^20).
 * THE CONVERSION'S EDGE: the quadrant number is an int.  Where |x * invpio2| >= 2^31 - 1 (|x| >= ~3.37e9), and for the infinities and NaN,
 * the conversion below would be undefined in C -- x86 gives INT_MIN there (a "sine" of 7e121), gfx950 saturates -- so the reduction refuses
 * such an x: r and t are NaN, and pm_sin, pm_cos and pm_tan return NaN, the same on every build.  The arguments are reachable (att_decode
 * turns any float of a CRC-valid packet into radians; rmcv_aim_input.motor_angle is unchecked), and att_canon / aim_canon carry the NaN out
 * through the ABI.  Below the edge nothing changed: the comparison is on the product the reduction computes anyway. */
PM_FN int pm_rem_pio2(double x, double* r_hi, double* r_lo)
{
    const double invpio2 = 0.6366197723675814;
    const double p1 = 1.5707963267341256;       /* first 33 bits of pi/2 */
    const double p2 = 6.077100506303966e-11;    /* next 33 bits          */
    const double p3 = 2.0222662487959506e-21;   /* the rest, as a double */
    double fn = x * invpio2;
    if (!(pm_fabs(fn) < 2147483647.0)) { /* 2^31 - 1; NaN fails the comparison too */
        *r_hi = __builtin_nan("");
        *r_lo = __builtin_nan("");
        return 0;
    }
    int n = (int)(fn < 0 ? fn - 0.5 : fn + 0.5);
    double dn = (double)n;
    double r = x - dn * p1;
    double w = dn * p2;
    double hi = r - w;
    double lo = (r - hi) - w;
    double t = dn * p3;
    double hi2 = hi - t;
    double lo2 = ((hi - hi2) - t) + lo;
    *r_hi = hi2;
    *r_lo = lo2;
    return n & 3;
}

PM_FN double pm_sin(double x)
{
    double r, t;
    if (pm_fabs(x) <= 0.7853981633974483) return pm_ksin(x, 0.0, 0);
    switch (pm_rem_pio2(x, &r, &t)) {
        case 0: return pm_ksin(r, t, 1);
        case 1: return pm_kcos(r, t);
        case 2: return -pm_ksin(r, t, 1);
        default: return -pm_kcos(r, t);
    }
}

PM_FN double pm_cos(double x)
{
    double r, t;
    if (pm_fabs(x) <= 0.7853981633974483) return pm_kcos(x, 0.0);
    switch (pm_rem_pio2(x, &r, &t)) {
        case 0: return pm_kcos(r, t);
        case 1: return -pm_ksin(r, t, 1);
        case 2: return -pm_kcos(r, t);
        default: return pm_ksin(r, t, 1);
    }
}

/* tan on [-pi/4, pi/4] (+eps); y is the tail of x; odd: the result is -1 / tan(x + y).  The classical kernel: the odd degree-27
 * polynomial split into two interleaved sums; above 0.6744 the argument is first reflected at pi/4 (tan(pi/4 - u) = 1 - 2 (u - u^2 / (1 + u))),
 * and -1 / w is computed from a head / tail split of w so that it keeps its last bit. */
PM_FN double pm_ktan(double x, double y, int odd)
{
    const double T0 = 3.33333333333334091986e-01, T1 = 1.33333333333201242699e-01, T2 = 5.39682539762260521377e-02,
                 T3 = 2.18694882948595424599e-02, T4 = 8.86323982359930005737e-03, T5 = 3.59207910759131235356e-03,
                 T6 = 1.45620945432529025516e-03, T7 = 5.88041240820264096874e-04, T8 = 2.46463134818469906812e-04,
                 T9 = 7.81794442939557092300e-05, T10 = 7.14072491382608190305e-05, T11 = -1.85586374855275456654e-05,
                 T12 = 2.59073051863633712884e-05;
    const double pio4 = 7.85398163397448278999e-01, pio4lo = 3.06161699786838301793e-17;
    const int big = pm_fabs(x) >= 0x1.59428p-1, neg = x < 0; /* 0.67434 */
    double z, r, v, w, s;
    if (big) {
        if (neg) { x = -x; y = -y; }
        x = (pio4 - x) + (pio4lo - y);
        y = 0.0;
    }
    z = x * x;
    w = z * z;
    r = T1 + w * (T3 + w * (T5 + w * (T7 + w * (T9 + w * T11))));
    v = z * (T2 + w * (T4 + w * (T6 + w * (T8 + w * (T10 + w * T12)))));
    s = z * x;
    r = y + z * (s * (r + v) + y) + s * T0;
    w = x + r;
    if (big) {
        s = odd ? -1.0 : 1.0;
        v = s - 2.0 * (x + (r - w * w / (w + s)));
        return neg ? -v : v;
    }
    if (!odd) return w;
    {
        const double w0 = pm_hi_word_only(w);
        const double a = -1.0 / w, a0 = pm_hi_word_only(a);
        v = r - (w0 - x); /* w0 + v = r + x */
        return a0 + a * (1.0 + a0 * w0 + a0 * v);
    }
}

/* tan for |x| < ~1e5 (pm_rem_pio2's domain), |error| < 1 ulp; NaN, the infinities and |x| >= ~3.37e9 (pm_rem_pio2: the conversion's edge)
 * give NaN, +-0 gives +-0.  (rm::DeltaHeight, src/mobility.cpp:48.) */
PM_FN double pm_tan(double x)
{
    double r, t;
    if (x - x != 0.0) return x - x; /* NaN, +-infinity */
    if (pm_fabs(x) <= 0.7853981633974483) {
        if (pm_fabs(x) < 7.450580596923828e-09) return x; /* 2^-27: tan(x) = x, and -0 stays -0 */
        return pm_ktan(x, 0.0, 0);
    }
    {
        const int n = pm_rem_pio2(x, &r, &t);
        return pm_ktan(r, t, n & 1);
    }
}

PM_FN double pm_atan(double x)
{
    const double hi0 = 4.63647609000806093515e-01, lo0 = 2.26987774529616870924e-17; /* atan(.5) */
    const double hi1 = 7.85398163397448278999e-01, lo1 = 3.06161699786838301793e-17; /* atan(1)  */
    const double hi2 = 9.82793723247329054082e-01, lo2 = 1.39033110312309984516e-17; /* atan(1.5)*/
    const double hi3 = 1.57079632679489655800e+00, lo3 = 6.12323399573676603587e-17; /* atan(inf)*/
    const double a0 = 3.33333333333329318027e-01, a1 = -1.99999999998764832476e-01,
                 a2 = 1.42857142725034663711e-01, a3 = -1.11111104054623557880e-01,
                 a4 = 9.09088713343650656196e-02, a5 = -7.69187620504482999495e-02,
                 a6 = 6.66107313738753120669e-02, a7 = -5.83357013379057348645e-02,
                 a8 = 4.97687799461593236017e-02, a9 = -3.65315727442169155270e-02,
                 a10 = 1.62858201153657823623e-02;
    int neg = x < 0;
    double ax = pm_fabs(x), hi = 0, lo = 0, z, w, s1, s2, res;
    int id;
    if (ax != ax) return x; /* NaN */
    if (ax >= 7.37869762948382064640e+19) { /* 2^66 */
        res = hi3 + lo3;
        return neg ? -res : res;
    }
    if (ax < 0.4375) {
        if (ax < 3.725290298461914e-09) return x; /* 2^-28: atan(x) = x */
        id = -1;
    } else if (ax < 1.1875) {
        if (ax < 0.6875) { id = 0; ax = (2.0 * ax - 1.0) / (2.0 + ax); hi = hi0; lo = lo0; }
        else             { id = 1; ax = (ax - 1.0) / (ax + 1.0);       hi = hi1; lo = lo1; }
    } else {
        if (ax < 2.4375) { id = 2; ax = (ax - 1.5) / (1.0 + 1.5 * ax); hi = hi2; lo = lo2; }
        else             { id = 3; ax = -1.0 / ax;                     hi = hi3; lo = lo3; }
    }
    z = ax * ax;
    w = z * z;
    s1 = z * (a0 + w * (a2 + w * (a4 + w * (a6 + w * (a8 + w * a10)))));
    s2 = w * (a1 + w * (a3 + w * (a5 + w * (a7 + w * a9))));
    if (id < 0) res = ax - ax * (s1 + s2);
    else        res = hi - ((ax * (s1 + s2) - lo) - ax);
    return neg ? -res : res;
}

/* atan2 for finite arguments (infinities/NaN are not produced on this path;
 * they are still mapped to something sensible).  Within 2 ulp of the true value (a correctly rounded quotient, pm_atan below 1 ulp, one
 * final subtraction; 1.26 measured) -- the "<= 1 ulp" of tests/test_pinned_math.py is the distance to glibc's result, not to the truth. */
PM_FN double pm_atan2(double y, double x)
{
    const double pi = 3.1415926535897931160e+00, pi_lo = 1.2246467991473531772e-16;
    const double pio2 = 1.5707963267948965580e+00;
    double z;
    if (x != x || y != y) return x + y;
    if (y == 0.0) {
        /* sign of zero is dropped: +-0/x -> 0 for x>=0, pi for x<0 */
        return (x < 0) ? pi : 0.0;
    }
    if (x == 0.0) return (y < 0) ? -pio2 : pio2;
    {
        double ay = pm_fabs(y), ax = pm_fabs(x);
        double q = ay / ax;
        z = pm_atan(q);
        if (x > 0) return (y < 0) ? -z : z;
        z = pi - (z - pi_lo);
        return (y < 0) ? -z : z;
    }
}

/* arccosine (IPPE's rotation-vector conversion, the solve_PnP row): the classic rational kernel R(z) ~ (asin(x) - x) / x^3
 * on |x| <= 0.5 and the sqrt reductions outside, |error| < 1 ulp.  sqrt is IEEE (correctly rounded) on host and device. */
PM_FN double pm_acos(double x)
{
    const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17, pi = 3.14159265358979311600e+00;
    const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
                 pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05,
                 qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
                 qS4 = 7.70381505559019352791e-02;
    double ax = pm_fabs(x), z, p, q, r, s, w;
    if (x != x) return x;
    if (ax >= 1.0) {
        if (x == 1.0) return 0.0;
        if (x == -1.0) return pi + 2.0 * pio2_lo;
        return (x - x) / (x - x); /* NaN */
    }
    if (ax < 0.5) {
        if (ax < 6.938893903907228e-18) return pio2_hi + pio2_lo; /* 2^-57 */
        z = x * x;
        p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        r = p / q;
        return pio2_hi - (x - (pio2_lo - x * r));
    }
    if (x < 0) {
        z = (1.0 + x) * 0.5;
        p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        s = __builtin_sqrt(z);
        r = p / q;
        w = r * s - pio2_lo;
        return pi - 2.0 * (s + w);
    }
    {
        double df, c;
        z = (1.0 - x) * 0.5;
        s = __builtin_sqrt(z);
        df = pm_hi_word_only(s);
        c = (z - df * df) / (s + df);
        p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        r = p / q;
        w = r * s + c;
        return 2.0 * (df + w);
    }
}

/* float variants: one evaluation in double, one rounding */
PM_FN float pm_atan2f(float y, float x) { return (float)pm_atan2((double)y, (double)x); }
PM_FN float pm_sinf(float x) { return (float)pm_sin((double)x); }
PM_FN float pm_cosf(float x) { return (float)pm_cos((double)x); }

/* fmod(x, 180) for 0 <= x < 720 -- each subtraction is exact (Sterbenz).  NaN comes back at once.  NOTHING ELSE MAY REACH IT: the loop
 * does not end for +infinity and runs ~1e298 times for 1e300 -- on a GPU that is a hang.  Its two callers (device_fit.h, direct_finish) pass
 * theta * 180 / pi and 90 + theta * 180 / pi, where theta is 0, pi / 2 or pi / 2 + 0.5 * pm_atan2(..): pm_atan2 returns a value in
 * [-pi, pi] or NaN for EVERY input (pm_atan is bounded by its hi + lo constants), so theta is in [0, pi] or NaN and the argument is below
 * 270.000001 or NaN. */
PM_FN double pm_fmod180(double x)
{
    while (x >= 180.0) x -= 180.0;
    return x;
}

/* ---- pow, for the gamma table of rm::CalcGamma (src/imgproc.cpp:43: pow(i / 255.0, gamma) * 255.0) -------------------------
 * pow(x, g) = exp(g * log(x)) for finite x > 0 (normal) and EVERY finite g, with pow(x, 0) = 1 and pow(0, g > 0) = 0; a result below
 * the normal range is 0 (pm_exp), so the table of a huge gamma is 0 .. 0 255, as the host libm's is.
 * log: x = 2^k m, m in [sqrt(1/2), sqrt(2)), log m = 2 atanh(s), s = (m - 1) / (m + 1), |s| <= 0.1716 (the odd series to s^23);
 * exp: y = n ln2 + r, |r| <= 0.347 (Cody-Waite in two pieces, Taylor to r^13).
 * log is below 1 ulp of the true value (0.78 measured; its sum starts from the exact m - 1, see the function), exp within 2 (1.09
 * measured); the product g * log(x) (up to 51 for the table's arguments) carries its rounding into the exponent, so the result's
 * relative error is up to (2.5 |g ln x| + 2) 2^-53 (tests/test_leaf_cpu.py), ~1.4e-14 for the table -- the table needs 1e-9 (no
 * pow(..) * 255 of the contract's gammas comes closer than 3e-7 to a rounding tie; tests/test_enhance_cpu.py compares all 256 entries
 * with the host libm's for every such gamma). */
PM_FN double pm_log(double x)
{
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    uint64_t u;
    int k;
    double m, f, s, z, p, hfsq, dk;
    __builtin_memcpy(&u, &x, 8);
    k = (int)(u >> 52) - 1023;
    u = (u & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull;
    __builtin_memcpy(&m, &u, 8);
    if (m > 1.4142135623730951) { m = m * 0.5; k = k + 1; }
    f = m - 1.0; /* exact */
    s = f / (2.0 + f);
    z = s * s;
    p = z * (1.0 / 3.0 + z * (1.0 / 5.0 + z * (1.0 / 7.0 + z * (1.0 / 9.0 + z * (1.0 / 11.0 + z * (1.0 / 13.0 + z * (1.0 / 15.0 +
        z * (1.0 / 17.0 + z * (1.0 / 19.0 + z * (1.0 / 21.0 + z * (1.0 / 23.0)))))))))));
    /* log m = 2 s + 2 s p, and 2 s = f - f^2 / 2 + s f^2 / 2: summed from the exact f, so that the rounding of s reaches only the small
     * terms (the classical arrangement; 2 s + 2 s p itself lost up to 1.9 ulp where k ln2 cancels half of it) */
    hfsq = 0.5 * f * f;
    dk = (double)k;
    if (k == 0) return f - (hfsq - s * (hfsq + 2.0 * p));
    return dk * ln2_hi - ((hfsq - (s * (hfsq + 2.0 * p) + dk * ln2_lo)) - f);
}

/* exp for every y that is not NaN: 0 below -708 (there the result leaves the normal range; its one caller rounds anything below
 * 0.5 / 255 to 0, so the subnormal range is flushed rather than computed), +infinity above 709; in between the result is a normal
 * number and so is the scale 2^n built below (-1022 <= n <= 1023). */
PM_FN double pm_exp(double y)
{
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10, inv_ln2 = 1.44269504088896338700e+00;
    double fn, dn, r, p, scale;
    int n;
    uint64_t u;
    if (y != y) return y;
    if (y < -708.0) return 0.0;
    if (y > 709.0) return __builtin_huge_val();
    fn = y * inv_ln2;
    n = (int)(fn < 0 ? fn - 0.5 : fn + 0.5);
    dn = (double)n;
    r = (y - dn * ln2_hi) - dn * ln2_lo;
    p = 1.0 / 6227020800.0;
    p = 1.0 / 479001600.0 + r * p;
    p = 1.0 / 39916800.0 + r * p;
    p = 1.0 / 3628800.0 + r * p;
    p = 1.0 / 362880.0 + r * p;
    p = 1.0 / 40320.0 + r * p;
    p = 1.0 / 5040.0 + r * p;
    p = 1.0 / 720.0 + r * p;
    p = 1.0 / 120.0 + r * p;
    p = 1.0 / 24.0 + r * p;
    p = 1.0 / 6.0 + r * p;
    p = 0.5 + r * p;
    p = 1.0 + r * p;
    p = 1.0 + r * p;
    u = (uint64_t)(n + 1023) << 52;
    __builtin_memcpy(&scale, &u, 8);
    return p * scale;
}

PM_FN double pm_pow(double x, double g)
{
    if (g == 0.0) return 1.0;
    if (x == 0.0) return 0.0;
    if (x == 1.0) return 1.0;
    return pm_exp(g * pm_log(x));
}

/* ---- hypot, for the Jacobi rotation of the device tracker's cv::solve(DECOMP_SVD) (device_track.h) -------------------------------
 * CORRECTLY ROUNDED over the whole finite range (round to nearest even, subnormal results included), C99 for 0, infinity and NaN.
 * The host libm's hypot is not correctly rounded and differs between machines, and a GPU has none: this one has a single right
 * answer, which tests/test_pinned_hypot.py checks against exact integer arithmetic.  Unlike the rest of this file it uses fma --
 * the explicit, exactly rounded one (__builtin_fma), never a contraction.
 * Method: both arguments scaled by a power of two into [2^-376, 2^500); x^2 and y^2 as exact double-double products; a candidate
 * from sqrt of their sum with one Newton correction (within an ulp); then the candidate is MOVED until x^2 + y^2 lies between the
 * squares of its two rounding boundaries, the sign of  x^2 + y^2 - (r +- half ulp)^2  being that of an eight-term sum computed
 * without error (Shewchuk's grow-expansion: the largest non-zero component of a non-overlapping expansion carries the sign).
 * A tie (a Pythagorean triple whose hypotenuse needs 54 bits) goes to the even neighbour.  When the larger argument is subnormal the
 * result's grid is 2^-1074 whatever its size: the arguments become integers and the candidate is rounded to an integer instead. */
#define PM_TS_(q, e)                          \
    {                                         \
        const double x_ = (q) + (e);          \
        const double bv_ = x_ - (q);          \
        const double av_ = x_ - bv_;          \
        (e) = ((q) - av_) + ((e) - bv_);      \
        (q) = x_;                             \
    }
/* the sign (-1, 0, 1) of t0 + ... + t7, exactly: no overflow, no underflow (the caller's scaling) */
PM_FN int pm_sign_sum8(double t0, double t1, double t2, double t3, double t4, double t5, double t6, double t7)
{
    double e0 = t0, e1, e2, e3, e4, e5, e6, e7, q;
    q = t1; PM_TS_(q, e0) e1 = q;
    q = t2; PM_TS_(q, e0) PM_TS_(q, e1) e2 = q;
    q = t3; PM_TS_(q, e0) PM_TS_(q, e1) PM_TS_(q, e2) e3 = q;
    q = t4; PM_TS_(q, e0) PM_TS_(q, e1) PM_TS_(q, e2) PM_TS_(q, e3) e4 = q;
    q = t5; PM_TS_(q, e0) PM_TS_(q, e1) PM_TS_(q, e2) PM_TS_(q, e3) PM_TS_(q, e4) e5 = q;
    q = t6; PM_TS_(q, e0) PM_TS_(q, e1) PM_TS_(q, e2) PM_TS_(q, e3) PM_TS_(q, e4) PM_TS_(q, e5) e6 = q;
    q = t7; PM_TS_(q, e0) PM_TS_(q, e1) PM_TS_(q, e2) PM_TS_(q, e3) PM_TS_(q, e4) PM_TS_(q, e5) PM_TS_(q, e6) e7 = q;
    q = e7 != 0 ? e7 : (e6 != 0 ? e6 : (e5 != 0 ? e5 : (e4 != 0 ? e4 : (e3 != 0 ? e3 : (e2 != 0 ? e2 : (e1 != 0 ? e1 : e0))))));
    return q > 0 ? 1 : (q < 0 ? -1 : 0);
}
#undef PM_TS_

PM_FN double pm_hypot(double x, double y)
{
    const double inf = __builtin_huge_val();
    const double p537 = 0x1p537, m537 = 0x1p-537; /* 2^537, 2^-537 */
    const double p600 = 0x1p600, m600 = 0x1p-600; /* 2^600, 2^-600 */
    const double p700 = 0x1p700, m700 = 0x1p-700; /* 2^700, 2^-700 */
    double ax = __builtin_fabs(x), ay = __builtin_fabs(y), un1 = 1.0, un2 = 1.0, r;
    double hx, lx, hy, ly, s, e;
    int fixed = 0, it;
    if (ax == inf || ay == inf) return inf;
    if (x != x || y != y) return x + y;
    if (ax < ay) { const double t = ax; ax = ay; ay = t; }
    if (ay == 0.0) return ax;
    if (ay <= ax * 0x1p-54) return ax; /* 2^-54 of the larger: y^2 / (2 x) is below 2^-55 of an ulp of x */
    if (ax >= 0x1p500) { /* 2^500 */
        ax *= m600; ay *= m600; un1 = p600;
    } else if (ax < 0x1p-1022) { /* subnormal: integers below 2^52 */
        ax = ax * p537 * p537; ay = ay * p537 * p537; un1 = m537; un2 = m537; fixed = 1;
    } else if (ax < 0x1p-250) { /* 2^-250 */
        ax *= p700; ay *= p700; un1 = m700;
    }
    hx = ax * ax; lx = __builtin_fma(ax, ax, -hx);
    hy = ay * ay; ly = __builtin_fma(ay, ay, -hy);
    s = hx + hy;
    e = ((hx - s) + hy) + (lx + ly);
    r = __builtin_sqrt(s);
    {
        const double rr = r * r, rl = __builtin_fma(r, r, -rr);
        r = r + (((s - rr) - rl) + e) / (2.0 * r);
    }
    if (fixed && r < 4503599627370496.0) r = (r + 4503599627370496.0) - 4503599627370496.0;
    for (it = 0; it < 4; it++) { /* the candidate is within an ulp: one move at most; the bound is a bound */
        uint64_t u;
        double up, dn, hu, hd, rr, rl;
        int odd, sg;
        __builtin_memcpy(&u, &r, 8);
        if (fixed) { up = r + 1.0; dn = r - 1.0; odd = (int)((uint64_t)r & 1u); }
        else {
            uint64_t v = u + 1;
            __builtin_memcpy(&up, &v, 8);
            v = u - 1;
            __builtin_memcpy(&dn, &v, 8);
            odd = (int)(u & 1u);
        }
        hu = (up - r) * 0.5;
        hd = (r - dn) * 0.5;
        rr = r * r;
        rl = __builtin_fma(r, r, -rr);
        sg = pm_sign_sum8(hx, lx, hy, ly, -rr, -rl, -(2.0 * r * hu), -(hu * hu));
        if (sg > 0 || (sg == 0 && odd)) { r = up; continue; }
        sg = pm_sign_sum8(hx, lx, hy, ly, -rr, -rl, 2.0 * r * hd, -(hd * hd));
        if (sg < 0 || (sg == 0 && odd)) { r = dn; continue; }
        break;
    }
    return r * un1 * un2;
}

#endif /* RMCV_PINNED_MATH_H */
