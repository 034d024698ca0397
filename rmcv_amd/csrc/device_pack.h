/*
 * device_pack.h -- the session recorder's lossless frame packer, host and device from the same source: the per-segment
 * rule (widths, mode, zigzag and its inverse), the sizes of a packed frame, and the sequential host packer / unpacker behind
 * rmcv_pack_host / rmcv_unpack_host.  What rm::debug::logger (include/debug.h:13-29, src/debug.cpp:9-41) keeps with FFV1 this keeps as
 * bit planes: a row is cut into segments of 256 bytes, a segment stores only the low b bits of its bytes (or of their zigzagged
 * differences to the byte `lag` before), one 64-bit word per bit and per byte-of-a-dword -- on the device one lane per dword and one
 * wave64 ballot per word (k_pack.hip).  Integers only: nothing here rounds.
 *
 * A packed frame of h rows of w_bytes bytes, S = ceil(w_bytes / 256):
 *   [ h * S header bytes, row-major: b | mode_predicted << 4 ][ 0 .. to a multiple of 8 ]
 *   [ h + 1 u32 row offsets into the payload area; entry h = its size ][ 0 .. to a multiple of 8 ]
 *   [ payloads in segment order: 32 * b bytes each; word (j, k), j < b outermost, k < 4: bit L = bit j of the coded byte 4 L + k ]
 * Bytes of the last segment beyond w_bytes are virtual: raw value 0, residual 0, never read.
 */
#ifndef RMCV_DEVICE_PACK_H
#define RMCV_DEVICE_PACK_H

#include <stdint.h>
#include <string.h>

#include "../../include/rmcv_abi.h"

#if defined(__HIPCC__)
#define PK_FN __host__ __device__ static inline
#else
#define PK_FN static inline
#endif

#define PACK_SEG 256      /* bytes of a segment: 64 lanes x one dword */
#define PACK_MODE_PRED 16 /* header bit: the segment stores zigzagged differences */

/* ---- the per-segment rule ---- */
/* bit length of a byte's value: 0 .. 8 */
PK_FN int pack_bitlen(unsigned x)
{
    int n = 0;
    while (x) { n++; x >>= 1; }
    return n;
}
/* r = (v - predecessor) mod 256 read as int8 s: ((s << 1) ^ (s >> 7)) & 0xFF, on unsigned values */
PK_FN unsigned pack_zigzag(unsigned r) { return ((r << 1) ^ ((r & 0x80u) ? 0xFFu : 0u)) & 0xFFu; }
PK_FN unsigned pack_unzigzag(unsigned z) { return ((z >> 1) ^ (0u - (z & 1u))) & 0xFFu; }
/* the header byte of a segment whose greatest byte has b_raw bits and whose greatest zigzagged difference has b_pred */
PK_FN unsigned pack_header(int b_raw, int b_pred) { return b_raw <= b_pred ? (unsigned)b_raw : ((unsigned)b_pred | PACK_MODE_PRED); }
/* a header byte a packer can have written: b <= 8, no other bits, and a predicted segment is narrower than its raw form (b <= 7) */
PK_FN int pack_header_ok(unsigned hb) { return (hb & 0xE0u) == 0 && (hb & 15u) <= 8 && !((hb & PACK_MODE_PRED) && (hb & 15u) == 8); }

/* ---- sizes ---- */
PK_FN int64_t pack_align8(int64_t x) { return (x + 7) & ~(int64_t)7; }
PK_FN int pack_segments(int w_bytes) { return (int)(((int64_t)w_bytes + PACK_SEG - 1) / PACK_SEG); }
PK_FN int64_t pack_header_bytes(int w_bytes, int h) { return pack_align8((int64_t)h * pack_segments(w_bytes)); }
PK_FN int64_t pack_table_bytes(int h) { return pack_align8(4 * ((int64_t)h + 1)); }
/* every segment at b = 8 */
PK_FN int64_t pack_bound(int w_bytes, int h)
{
    return pack_header_bytes(w_bytes, h) + pack_table_bytes(h) + (int64_t)PACK_SEG * h * pack_segments(w_bytes);
}
/* the geometry a packed frame can have: row offsets are u32 */
PK_FN int pack_geometry_ok(int w_bytes, int h, int lag)
{
    return w_bytes >= 1 && h >= 1 && lag >= 1 && lag <= 4 && (int64_t)PACK_SEG * h * pack_segments(w_bytes) < ((int64_t)1 << 31);
}
/* the lag of a plane of frames: the distance in bytes to the previous sample of the same kind */
PK_FN int pack_lag(int input_format, int sample_bits) { return input_format == RMCV_INPUT_BGR ? 3 : (sample_bits == 16 ? 4 : 2); }

/* ---- the sequential host form ---- */
static inline uint32_t pack_get32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static inline void pack_put32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

/* segment s of a row: its header byte, and the 256 coded values of the chosen mode */
static inline unsigned pack_segment_host(const uint8_t* row, int w_bytes, int s, int lag, uint8_t coded[PACK_SEG])
{
    uint8_t z[PACK_SEG];
    unsigned or_v = 0, or_z = 0;
    for (int t = 0; t < PACK_SEG; t++) {
        const int i = s * PACK_SEG + t;
        unsigned v = 0, zz = 0;
        if (i < w_bytes) {
            v = row[i];
            zz = pack_zigzag((v - (i >= lag ? row[i - lag] : 0u)) & 0xFFu);
        }
        coded[t] = (uint8_t)v;
        z[t] = (uint8_t)zz;
        or_v |= v;
        or_z |= zz;
    }
    const unsigned hb = pack_header(pack_bitlen(or_v), pack_bitlen(or_z));
    if (hb & PACK_MODE_PRED) memcpy(coded, z, PACK_SEG);
    return hb;
}

/* pack h rows of w_bytes bytes, `stride` apart, into out[0 .. cap): RMCV_ERR_CAPACITY when it does not fit (*size says what it needs) */
static inline int pack_host(const uint8_t* src, int w_bytes, int h, int64_t stride, int lag, uint8_t* out, int64_t cap, int64_t* size)
{
    if (!src || !out || !pack_geometry_ok(w_bytes, h, lag) || stride < w_bytes || cap < 0) return RMCV_ERR_BAD_ARG;
    const int S = pack_segments(w_bytes);
    const int64_t H = pack_header_bytes(w_bytes, h), T = pack_table_bytes(h);
    if (cap < H + T) {
        if (size) *size = pack_bound(w_bytes, h);
        return RMCV_ERR_CAPACITY;
    }
    uint8_t coded[PACK_SEG];
    memset(out, 0, (size_t)(H + T));
    int64_t total = 0;
    for (int y = 0; y < h; y++) {
        pack_put32(out + H + 4 * (int64_t)y, (uint32_t)total);
        for (int s = 0; s < S; s++) {
            const unsigned hb = pack_segment_host(src + y * stride, w_bytes, s, lag, coded);
            out[(int64_t)y * S + s] = (uint8_t)hb;
            total += 32 * (int64_t)(hb & 15u);
        }
    }
    pack_put32(out + H + 4 * (int64_t)h, (uint32_t)total);
    if (size) *size = H + T + total;
    if (cap < H + T + total) return RMCV_ERR_CAPACITY;
    uint8_t* p = out + H + T;
    for (int y = 0; y < h; y++)
        for (int s = 0; s < S; s++) {
            const int b = (int)(pack_segment_host(src + y * stride, w_bytes, s, lag, coded) & 15u);
            for (int j = 0; j < b; j++)
                for (int k = 0; k < 4; k++) {
                    uint64_t word = 0;
                    for (int L = 0; L < 64; L++) word |= (uint64_t)((coded[4 * L + k] >> j) & 1u) << L;
                    for (int q = 0; q < 8; q++) *p++ = (uint8_t)(word >> (8 * q));
                }
        }
    return RMCV_OK;
}

/* whether buf[0 .. len) is a packed frame of h rows of w_bytes bytes: header bytes a packer can have written, zero padding, a row table
 * that is the running sum of the header's widths, and len exactly what they add up to.  Reads nothing outside the buffer. */
static inline int pack_check_host(const uint8_t* buf, int64_t len, int w_bytes, int h)
{
    if (!buf || len < 0 || !pack_geometry_ok(w_bytes, h, 1)) return RMCV_ERR_BAD_ARG;
    const int S = pack_segments(w_bytes);
    const int64_t H = pack_header_bytes(w_bytes, h), T = pack_table_bytes(h);
    if (len < H + T) return RMCV_ERR_BAD_ARG;
    for (int64_t i = (int64_t)h * S; i < H; i++) if (buf[i]) return RMCV_ERR_BAD_ARG;
    for (int64_t i = 4 * ((int64_t)h + 1); i < T; i++) if (buf[H + i]) return RMCV_ERR_BAD_ARG;
    int64_t total = 0;
    for (int y = 0; y <= h; y++) {
        if (pack_get32(buf + H + 4 * (int64_t)y) != (uint64_t)total) return RMCV_ERR_BAD_ARG;
        if (y == h) break;
        for (int s = 0; s < S; s++) {
            const unsigned hb = buf[(int64_t)y * S + s];
            if (!pack_header_ok(hb)) return RMCV_ERR_BAD_ARG;
            total += 32 * (int64_t)(hb & 15u);
        }
    }
    return len == H + T + total ? RMCV_OK : RMCV_ERR_BAD_ARG;
}

/* the inverse of pack_host: bytes beyond w_bytes of a destination row are left alone */
static inline int unpack_host(const uint8_t* buf, int64_t len, int w_bytes, int h, int lag, uint8_t* dst, int64_t stride)
{
    if (!dst || lag < 1 || lag > 4 || stride < w_bytes) return RMCV_ERR_BAD_ARG;
    const int rc = pack_check_host(buf, len, w_bytes, h);
    if (rc) return rc;
    const int S = pack_segments(w_bytes);
    const uint8_t* p = buf + pack_header_bytes(w_bytes, h) + pack_table_bytes(h);
    for (int y = 0; y < h; y++) {
        uint8_t* row = dst + y * stride;
        for (int s = 0; s < S; s++) {
            const unsigned hb = buf[(int64_t)y * S + s];
            const int b = (int)(hb & 15u);
            uint8_t coded[PACK_SEG] = {0};
            for (int j = 0; j < b; j++)
                for (int k = 0; k < 4; k++) {
                    uint64_t word = 0;
                    for (int q = 0; q < 8; q++) word |= (uint64_t)(*p++) << (8 * q);
                    for (int L = 0; L < 64; L++) coded[4 * L + k] |= (uint8_t)(((word >> L) & 1u) << j);
                }
            for (int t = 0; t < PACK_SEG; t++) {
                const int i = s * PACK_SEG + t;
                if (i >= w_bytes) break;
                if (hb & PACK_MODE_PRED) row[i] = (uint8_t)(pack_unzigzag(coded[t]) + (i >= lag ? row[i - lag] : 0u));
                else row[i] = coded[t];
            }
        }
    }
    return RMCV_OK;
}
#endif /* RMCV_DEVICE_PACK_H */
