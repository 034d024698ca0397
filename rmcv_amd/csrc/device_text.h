/*
 * device_text.h -- the label pass over a finished view, host and device from the same source: what rm::debug::draw_armours
 * writes next to every armour (src/debug.cpp:53-57)
 *     to_string(identity) + ": " + to_string(x) + ", " + to_string(y) + ", " + to_string(z)
 * and, for a tracked run, every target's quadrilateral with the same line followed by ", " + to_string(lost_count).
 *
 * Here: the two number formats (no libc on either side), the line's characters, the library's own 5 x 7 glyphs, the placement of a glyph's
 * pixels, the mapping of a vertex into the view, and the draw of one armour label / one track as a sequence of put(x, y) calls.  Integer
 * arithmetic throughout but for the clip of device_view.h.  The deviations from the reference: rmcv_abi.h, "view labels".
 *
 * A number is written RIGHT-ALIGNED into a field of LABEL_FIELD characters; its text is field[start .. LABEL_FIELD).  The caller owns the
 * field: a char array on the host, a row of LDS on the device (no digit is ever kept in an indexed private array).
 */
#ifndef RMCV_DEVICE_TEXT_H
#define RMCV_DEVICE_TEXT_H

#include <stdint.h>
#include <string.h>

#include "device_view.h"

#define LABEL_FIELD 24     /* >= the longest number: '-' + 15 digits + '.' + 6 digits = 23 */
#define LABEL_FIELDS 5     /* identity, x, y, z, lost_count */
#define LABEL_SCALE_MAX 8
#define LABEL_GLYPH_W 5
#define LABEL_GLYPH_H 7
#define LABEL_ADVANCE 6    /* columns from one character to the next, in glyph pixels */
static_assert(11 + 2 + 3 * 23 + 2 * 2 + 2 + 11 <= RMCV_LABEL_MAX_CHARS, "a track's line: dec : f6 , f6 , f6 , dec");

/* dec(i) = std::to_string(int32): returns start */
VIEW_FN int label_dec(int32_t v, char* field)
{
    uint32_t u = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    int at = LABEL_FIELD;
    do {
        field[--at] = (char)('0' + u % 10u);
        u /= 10u;
    } while (u);
    if (v < 0) field[--at] = '-';
    return at;
}

VIEW_FN int label_word(int neg, char a, char b, char c, char* field)
{
    field[LABEL_FIELD - 3] = a, field[LABEL_FIELD - 2] = b, field[LABEL_FIELD - 1] = c;
    if (!neg) return LABEL_FIELD - 3;
    field[LABEL_FIELD - 4] = '-';
    return LABEL_FIELD - 4;
}

/* f6(v) = std::to_string(double) = "%f" for finite |v| < 1e15: six decimals, rounded half to even ON THE EXACT BINARY VALUE, in integers.
 *   v = m 2^e, m < 2^53.  P = m 10^6 < 2^73 as two 64-bit halves; |v| < 1e15 < 2^50 means e <= -3 (a subnormal: e = -1074), so
 *   N = round_half_even(P / 2^s), s = -e >= 3, is the number of millionths: N < 10^21 < 2^70.  N / 10^6 and N mod 10^6 by long division
 *   over 32-bit limbs (the running remainder is < 10^6 < 2^20, so every partial dividend fits 52 bits).
 * nan (any sign), inf / -inf, and big / -big for a finite |v| >= 1e15 are the stated deviations.  Returns start. */
VIEW_FN int label_f6(double v, char* field)
{
    uint64_t bits;
    memcpy(&bits, &v, 8);
    const int neg = (int)(bits >> 63), be = (int)(bits >> 52) & 0x7FF;
    const uint64_t frac = bits & 0xFFFFFFFFFFFFFull;
    if (be == 0x7FF) return frac ? label_word(0, 'n', 'a', 'n', field) : label_word(neg, 'i', 'n', 'f', field);
    /* 1e15 = 0x430C6BF526340000 exactly: for finite values the order of the magnitudes is the order of their bit patterns */
    if ((bits & 0x7FFFFFFFFFFFFFFFull) >= 0x430C6BF526340000ull) return label_word(neg, 'b', 'i', 'g', field);
    const uint64_t m = be ? frac | (1ull << 52) : frac;
    const int s = be ? 1075 - be : 1074; /* v = m / 2^s, 3 <= s <= 1074 */
    /* P = m * 10^6 */
    const uint64_t a = (m & 0xFFFFFFFFull) * 1000000ull, b = (m >> 32) * 1000000ull; /* < 2^52, < 2^41 */
    uint64_t lo = (b << 32) + a;
    uint64_t hi = (b >> 32) + (lo < a ? 1u : 0u);
    /* N = round_half_even(P >> s) */
    uint64_t nlo, nhi;
    if (s >= 75) { /* P < 2^73 <= half of 2^s: below the tie */
        nlo = nhi = 0;
    } else {
        uint64_t rem_hi, rem_lo, half_hi, half_lo; /* P mod 2^s and 2^(s - 1) */
        if (s >= 64) {
            const int t = s - 64; /* 0 .. 10 */
            nlo = hi >> t, nhi = 0;
            rem_hi = t ? hi & ((1ull << t) - 1) : 0, rem_lo = lo;
            half_hi = t ? 1ull << (t - 1) : 0, half_lo = t ? 0 : 1ull << 63;
        } else {
            nlo = (lo >> s) | (hi << (64 - s)), nhi = hi >> s;
            rem_hi = 0, rem_lo = lo & ((1ull << s) - 1);
            half_hi = 0, half_lo = 1ull << (s - 1);
        }
        const int above = rem_hi > half_hi || (rem_hi == half_hi && rem_lo > half_lo);
        const int tie = rem_hi == half_hi && rem_lo == half_lo;
        if (above || (tie && (nlo & 1))) {
            nlo += 1;
            nhi += nlo == 0;
        }
    }
    /* N = (nhi, nlo), nhi < 64: integer part and millionths */
    uint64_t cur = (nhi << 32) | (nlo >> 32); /* nhi / 10^6 = 0 */
    const uint64_t q1 = cur / 1000000ull;
    cur = ((cur % 1000000ull) << 32) | (nlo & 0xFFFFFFFFull);
    const uint64_t q2 = cur / 1000000ull;
    uint32_t f = (uint32_t)(cur % 1000000ull);
    uint64_t ip = (q1 << 32) | q2; /* < 10^15 */
    int at = LABEL_FIELD;
    for (int i = 0; i < 6; i++) {
        field[--at] = (char)('0' + f % 10u);
        f /= 10u;
    }
    field[--at] = '.';
    do {
        field[--at] = (char)('0' + (int)(ip % 10ull));
        ip /= 10ull;
    } while (ip);
    if (neg) field[--at] = '-';
    return at;
}

/* character k of the line made of n_fields numbers (fields: n_fields rows of LABEL_FIELD characters, starts: their starts): the first
 * two are joined by ": ", the others by ", ".  0: the line has no character k. */
VIEW_FN int label_char_at(const char* fields, const int* starts, int n_fields, int k)
{
    for (int i = 0; i < n_fields; i++) {
        if (i) {
            if (k == 0) return i == 1 ? ':' : ',';
            if (k == 1) return ' ';
            k -= 2;
        }
        const int len = LABEL_FIELD - starts[i];
        if (k < len) return fields[i * LABEL_FIELD + starts[i] + k];
        k -= len;
    }
    return 0;
}

/* ---- the font: the library's own 5 x 7 glyphs, drawn here by hand, for exactly the characters a line can contain ---------------------
 * A glyph is 7 rows, top to bottom, of 5 bits: the LEFT column is bit 4, so that a row reads as it is written below.  Packed: row r in
 * bits 5 (6 - r) .. 5 (6 - r) + 4. */
#define LABEL_G(r0, r1, r2, r3, r4, r5, r6) \
    (((uint64_t)(r0) << 30) | ((uint64_t)(r1) << 25) | ((uint64_t)(r2) << 20) | ((uint64_t)(r3) << 15) | ((uint64_t)(r4) << 10) | ((uint64_t)(r5) << 5) | (uint64_t)(r6))
/* the packed glyph of a character; ~0: the character is outside the set */
VIEW_FN uint64_t label_glyph(int ch)
{
    switch (ch) {
    case '0': return LABEL_G(0b01110,
                             0b10001,
                             0b10011,
                             0b10101,
                             0b11001,
                             0b10001,
                             0b01110);
    case '1': return LABEL_G(0b00100,
                             0b01100,
                             0b00100,
                             0b00100,
                             0b00100,
                             0b00100,
                             0b01110);
    case '2': return LABEL_G(0b01110,
                             0b10001,
                             0b00001,
                             0b00010,
                             0b00100,
                             0b01000,
                             0b11111);
    case '3': return LABEL_G(0b11110,
                             0b00001,
                             0b00001,
                             0b01110,
                             0b00001,
                             0b00001,
                             0b11110);
    case '4': return LABEL_G(0b00010,
                             0b00110,
                             0b01010,
                             0b10010,
                             0b11111,
                             0b00010,
                             0b00010);
    case '5': return LABEL_G(0b11111,
                             0b10000,
                             0b11110,
                             0b00001,
                             0b00001,
                             0b10001,
                             0b01110);
    case '6': return LABEL_G(0b00110,
                             0b01000,
                             0b10000,
                             0b11110,
                             0b10001,
                             0b10001,
                             0b01110);
    case '7': return LABEL_G(0b11111,
                             0b00001,
                             0b00010,
                             0b00100,
                             0b01000,
                             0b01000,
                             0b01000);
    case '8': return LABEL_G(0b01110,
                             0b10001,
                             0b10001,
                             0b01110,
                             0b10001,
                             0b10001,
                             0b01110);
    case '9': return LABEL_G(0b01110,
                             0b10001,
                             0b10001,
                             0b01111,
                             0b00001,
                             0b00010,
                             0b01100);
    case '-': return LABEL_G(0b00000,
                             0b00000,
                             0b00000,
                             0b11111,
                             0b00000,
                             0b00000,
                             0b00000);
    case '.': return LABEL_G(0b00000,
                             0b00000,
                             0b00000,
                             0b00000,
                             0b00000,
                             0b01100,
                             0b01100);
    case ':': return LABEL_G(0b00000,
                             0b01100,
                             0b01100,
                             0b00000,
                             0b01100,
                             0b01100,
                             0b00000);
    case ',': return LABEL_G(0b00000,
                             0b00000,
                             0b00000,
                             0b00000,
                             0b01100,
                             0b00100,
                             0b01000);
    case ' ': return 0;
    case 'n': return LABEL_G(0b00000,
                             0b00000,
                             0b10110,
                             0b11001,
                             0b10001,
                             0b10001,
                             0b10001);
    case 'a': return LABEL_G(0b00000,
                             0b00000,
                             0b01110,
                             0b00001,
                             0b01111,
                             0b10001,
                             0b01111);
    case 'i': return LABEL_G(0b00100,
                             0b00000,
                             0b01100,
                             0b00100,
                             0b00100,
                             0b00100,
                             0b01110);
    case 'f': return LABEL_G(0b00110,
                             0b01001,
                             0b01000,
                             0b11100,
                             0b01000,
                             0b01000,
                             0b01000);
    case 'b': return LABEL_G(0b10000,
                             0b10000,
                             0b10110,
                             0b11001,
                             0b10001,
                             0b10001,
                             0b11110);
    case 'g': return LABEL_G(0b00000,
                             0b00000,
                             0b01111,
                             0b10001,
                             0b01111,
                             0b00001,
                             0b01110);
    default: return ~0ull;
    }
}
VIEW_FN int label_glyph_row(uint64_t g, int r) { return (int)(g >> (5 * (6 - r))) & 31; }

/* ---- placement ---------------------------------------------------------------------------------------------------------------------- */
/* floor(p n_dst / n_src): a coordinate of the frame's geometry (w or h = n_src >= 1) in the view (vw or vh = n_dst); |p| < 2^31 */
VIEW_FN int64_t label_map(int64_t p, int n_dst, int n_src)
{
    const int64_t a = p * n_dst, q = a / n_src;
    return q - (a % n_src != 0 && a < 0);
}

/* character k of a line anchored at (ax, ay) -- the text's bottom-left, as putText's origin -- at scale s: a set bit at glyph column c
 * (0 left), row r (0 top) fills the s x s block at x = ax + (6 k + c) s, y = ay - (7 - r) s; every pixel clipped to the view */
template <typename Put>
VIEW_FN void label_blit(int vw, int vh, int64_t ax, int64_t ay, int s, int k, int ch, Put put)
{
    const uint64_t g = label_glyph(ch);
    if (g == 0 || g == ~0ull) return;
    const int64_t x0 = ax + (int64_t)LABEL_ADVANCE * k * s, y0 = ay - (int64_t)LABEL_GLYPH_H * s;
    if (x0 >= vw || x0 + (int64_t)LABEL_GLYPH_W * s <= 0 || y0 >= vh || ay <= 0) return; /* the whole cell is outside */
    for (int r = 0; r < LABEL_GLYPH_H; r++) {
        const int row = label_glyph_row(g, r);
        if (!row) continue;
        for (int c = 0; c < LABEL_GLYPH_W; c++) {
            if (!(row >> (4 - c) & 1)) continue;
            for (int dy = 0; dy < s; dy++) {
                const int64_t y = y0 + (int64_t)r * s + dy;
                if (y < 0 || y >= vh) continue;
                for (int dx = 0; dx < s; dx++) {
                    const int64_t x = x0 + (int64_t)c * s + dx;
                    if (x >= 0 && x < vw) put((int)x, (int)y);
                }
            }
        }
    }
}

/* a vertex (float, in the coordinates the caller names: cvRound, half to even) moved by (-ox, -oy) into the geometry's coordinates and
 * mapped into the view; 0: not finite or of magnitude >= 2^30 -- its label or quadrilateral is skipped */
VIEW_FN int label_anchor(const float* v, int ox, int oy, int w, int h, int vw, int vh, int64_t* ax, int64_t* ay)
{
    int px, py;
    if (!view_coord(v[0], &px) || !view_coord(v[1], &py)) return 0;
    *ax = label_map((int64_t)px - ox, vw, w);
    *ay = label_map((int64_t)py - oy, vh, h);
    return 1;
}

/* a segment between two view positions, through device_view.h's clip and line iterator with the view as the canvas (a mapped position
 * may lie beyond int32: the clip runs on the 64-bit values, the iterator on what is left inside) */
template <typename Put>
VIEW_FN void label_segment(int vw, int vh, int64_t x1, int64_t y1, int64_t x2, int64_t y2, Put put)
{
    if (x1 < 0 || x1 >= vw || x2 < 0 || x2 >= vw || y1 < 0 || y1 >= vh || y2 < 0 || y2 >= vh)
        if (!view_clip_line(vw, vh, &x1, &y1, &x2, &y2)) return;
    view_line(vw, vh, (int)x1, (int)y1, (int)x2, (int)y2, put);
}

/* where a track's line takes its position from: the filter's posterior once initialised, else the observation's (the aim step's rule) */
VIEW_FN double label_track_coord(const rmcv_track* t, int i) { return t->initialized ? t->state_post[i] : t->position[i]; }

/* ---- the host side: the lines as strings, and the sequential restatement ----------------------------------------------------------- */
/* the line into out[0 .. cap): its length (without the terminator), or -1 when cap is too small for it and the terminator */
static inline int label_line_host(const char* fields, const int* starts, int n_fields, char* out, int cap)
{
    int n = 0;
    for (int ch; (ch = label_char_at(fields, starts, n_fields, n)) != 0; n++)
        if (n < cap) out[n] = (char)ch;
    if (n >= cap) return -1;
    out[n] = 0;
    return n;
}
struct label_fields {
    char f[LABEL_FIELDS * LABEL_FIELD];
    int start[LABEL_FIELDS];
};
static inline void label_fields_armour(label_fields* L, int32_t identity, const double* pos)
{
    L->start[0] = label_dec(identity, L->f);
    for (int i = 0; i < 3; i++) L->start[1 + i] = label_f6(pos ? pos[i] : 0.0, L->f + (1 + i) * LABEL_FIELD);
}
static inline void label_fields_track(label_fields* L, const rmcv_track* t)
{
    L->start[0] = label_dec(t->identity, L->f);
    for (int i = 0; i < 3; i++) L->start[1 + i] = label_f6(label_track_coord(t, i), L->f + (1 + i) * LABEL_FIELD);
    L->start[4] = label_dec(t->lost_count, L->f + 4 * LABEL_FIELD);
}

static inline const char* label_check_host(const uint8_t* view, int vw, int vh, int stride, int w, int h, int scale, const rmcv_armour* armours, int n_armours,
                                           const rmcv_track* tracks, const float* last_vertices, int n_tracks)
{
    if (!view) return "null view";
    if (vw < 1 || vh < 1) return "the view needs vw >= 1 and vh >= 1";
    if (stride < 3 * (int64_t)vw) return "stride < 3 vw";
    if (w < 1 || h < 1) return "the geometry needs w >= 1 and h >= 1";
    if (scale < 1 || scale > LABEL_SCALE_MAX) return "scale outside 1 .. 8";
    if (n_armours < 0 || n_tracks < 0) return "negative list length";
    if ((n_armours && !armours) || (n_tracks && (!tracks || !last_vertices))) return "null list";
    return nullptr;
}

/* everything of the tracks first (magenta), then the armours' lines (yellow), drawn in place */
static inline void label_host(uint8_t* view, int vw, int vh, int stride, int w, int h, int scale, const rmcv_armour* armours, const int32_t* identities,
                              const double* positions, int n_armours, const rmcv_track* tracks, const float* last_vertices, int n_tracks, int x_eff, int y_eff)
{
    uint8_t bgr[3] = {255, 0, 255};
    auto put = [&](int x, int y) {
        uint8_t* p = view + (size_t)y * stride + 3 * (size_t)x;
        p[0] = bgr[0], p[1] = bgr[1], p[2] = bgr[2];
    };
    label_fields L;
    for (int t = 0; t < n_tracks; t++) {
        const float* q = last_vertices + (size_t)t * 8;
        int64_t x[4], y[4];
        int ok = 0; // bit j: vertex j is drawable.  The quadrilateral needs all four, the line its anchor, vertex 0
        for (int j = 0; j < 4; j++) ok |= label_anchor(q + 2 * j, x_eff, y_eff, w, h, vw, vh, &x[j], &y[j]) << j;
        if (ok == 15)
            for (int j = 0; j < 4; j++) label_segment(vw, vh, x[j], y[j], x[(j + 1) & 3], y[(j + 1) & 3], put);
        if (!(ok & 1)) continue;
        label_fields_track(&L, tracks + t);
        for (int k = 0, ch; (ch = label_char_at(L.f, L.start, 5, k)) != 0; k++) label_blit(vw, vh, x[0], y[0], scale, k, ch, put);
    }
    bgr[0] = 0, bgr[1] = 255, bgr[2] = 255;
    for (int i = 0; i < n_armours; i++) {
        int64_t ax, ay;
        if (!label_anchor(armours[i].vertices[0], 0, 0, w, h, vw, vh, &ax, &ay)) continue;
        label_fields_armour(&L, identities ? identities[i] : -1, positions ? positions + 3 * (size_t)i : nullptr);
        for (int k = 0, ch; (ch = label_char_at(L.f, L.start, 4, k)) != 0; k++) label_blit(vw, vh, ax, ay, scale, k, ch, put);
    }
}

#endif /* RMCV_DEVICE_TEXT_H */
