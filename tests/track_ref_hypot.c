/*
 * track_ref_hypot.c -- TEST INFRASTRUCTURE: trk_ref_hypot, a correctly rounded hypot written independently of
 * rmcv_amd/csrc/pinned_math.h (which it does not include): integers only.  Both arguments become 53-bit integer mantissas with
 * exponents, x^2 + y^2 an exact 256-bit integer, its integer square root (digit by digit) and remainder give the 53-bit result,
 * rounded to nearest even.  tests/track_ref.py compiles oracle/rmcv_oracle_track.c with -Dhypot=trk_ref_hypot against this file:
 * the reference of the device tracker's tests is the oracle's own source with only hypot replaced.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

typedef unsigned __int128 u128;
typedef struct { u128 hi, lo; } u256;

static u256 u256_add(u256 a, u256 b)
{
    u256 r;
    r.lo = a.lo + b.lo;
    r.hi = a.hi + b.hi + (r.lo < a.lo);
    return r;
}
static u256 u256_sub(u256 a, u256 b)
{
    u256 r;
    r.lo = a.lo - b.lo;
    r.hi = a.hi - b.hi - (a.lo < b.lo);
    return r;
}
static int u256_ge(u256 a, u256 b) { return a.hi > b.hi || (a.hi == b.hi && a.lo >= b.lo); }
static int u256_zero(u256 a) { return a.hi == 0 && a.lo == 0; }
static u256 u256_shr(u256 a, int n) /* n = 1 or 2 */
{
    u256 r;
    r.lo = (a.lo >> n) | (a.hi << (128 - n));
    r.hi = a.hi >> n;
    return r;
}
static u256 u256_shl(u256 a, int n) /* 0 <= n < 128 */
{
    u256 r;
    if (n == 0) return a;
    r.hi = (a.hi << n) | (a.lo >> (128 - n));
    r.lo = a.lo << n;
    return r;
}

/* |v| = m * 2^e, m < 2^53, e >= -1074 */
static void split(double v, uint64_t* m, int* e)
{
    uint64_t u;
    memcpy(&u, &v, 8);
    const int be = (int)((u >> 52) & 0x7FF);
    *m = (u & 0x000FFFFFFFFFFFFFull) | (be ? 0x0010000000000000ull : 0);
    *e = (be ? be : 1) - 1075;
}

static int bitlen(u128 v)
{
    int n = 0;
    while (v) { n++; v >>= 1; }
    return n;
}

/* the argument pairs of the calls made, for the fixed list of tests/golden/track_hypot_pairs.json (buf: 2 * cap doubles; NULL: off) */
static double* g_log;
static int g_log_cap, g_log_n;
void trk_ref_hypot_record(double* buf, int cap) { g_log = buf; g_log_cap = cap; g_log_n = 0; }
int trk_ref_hypot_recorded(void) { return g_log_n; }

double trk_ref_hypot(double x, double y)
{
    if (g_log && g_log_n < g_log_cap) {
        g_log[2 * g_log_n] = x;
        g_log[2 * g_log_n + 1] = y;
        g_log_n++;
    }
    if (isinf(x) || isinf(y)) return INFINITY;
    if (isnan(x) || isnan(y)) return x + y;
    double a = fabs(x), b = fabs(y);
    if (a < b) { const double t = a; a = b; b = t; }
    if (b == 0) return a;
    int fa, fb;
    frexp(a, &fa);
    frexp(b, &fb);
    if (fa - fb > 60) return a; /* b^2 / (2 a) < 2^-66 ulp of a */
    uint64_t ma, mb;
    int ea, eb;
    split(a, &ma, &ea);
    split(b, &mb, &eb);
    const int d = ea - eb; /* 0 .. 60 */
    u256 A = {0, (u128)ma * ma}, B = {0, (u128)mb * mb};
    int sh = 2 * d;
    while (sh > 0) { const int k = sh > 100 ? 100 : sh; A = u256_shl(A, k); sh -= k; }
    u256 num = u256_add(A, B); /* (hypot / 2^eb)^2, below 2^228 */
    u256 res = {0, 0}, bit = {(u128)1 << 126, 0};
    while (!u256_ge(num, bit)) bit = u256_shr(bit, 2);
    while (!u256_zero(bit)) {
        const u256 t = u256_add(res, bit);
        if (u256_ge(num, t)) {
            num = u256_sub(num, t);
            res = u256_add(u256_shr(res, 1), bit);
        } else res = u256_shr(res, 1);
        bit = u256_shr(bit, 2);
    }
    /* res = floor(sqrt), num = the remainder; res < 2^114 */
    const u128 T = res.lo;
    const int L = bitlen(T);
    u128 q;
    int shift = 0;
    if (L <= 53) {
        q = T + (u256_ge(num, (u256){0, T + 1}) ? 1 : 0); /* fraction above one half <=> remainder > T (never a tie) */
    } else {
        shift = L - 53;
        const u128 half = (u128)1 << (shift - 1), low = T & (((u128)1 << shift) - 1);
        q = T >> shift;
        if (low > half || (low == half && (!u256_zero(num) || (q & 1)))) q++;
    }
    return ldexp((double)(uint64_t)q, eb + shift);
}

void trk_ref_hypot_n(const double* x, const double* y, double* out, int n)
{
    for (int i = 0; i < n; i++) out[i] = trk_ref_hypot(x[i], y[i]);
}
