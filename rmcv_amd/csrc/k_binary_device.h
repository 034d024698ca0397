// k_binary_device.h -- what the pixel kernels share (k_binary.hip, k_binary_ws.inc, k_binary_enh.hip): the build knobs, the strip height,
// the packed threshold of 16 pixels -- plain (thresh16) and through a frame's gamma table (thresh16_m) -- and the raw-buffer types.
#pragma once
#include "rmcv_internal.h"

namespace rmcv {


#ifndef RMCV_SR
#define RMCV_SR 32
#endif
#ifndef RMCV_K1_UNROLL
#define RMCV_K1_UNROLL 4
#endif
#ifndef RMCV_K1_STAUX
#define RMCV_K1_STAUX 2 // cache-policy bits of the byte-image stores (2 = nt)
#endif
#ifndef RMCV_K1_PLAIN_PLAUX
#define RMCV_K1_PLAIN_PLAUX 0 // cache-policy bits of the bit-plane stores (plain: the sparse kernel of the same batch finds the words in L2)
#endif
#ifndef RMCV_K1_HALOAUX
#define RMCV_K1_HALOAUX 0 // cache-policy bits of the loads of the row quads a strip shares with its neighbours (0 = cacheable: the neighbour finds them in L2)
#endif
#ifndef RMCV_K1_LDAUX
#define RMCV_K1_LDAUX 2 // cache-policy bits of the frame loads that no other workgroup shares (2 = nt)
#endif
static constexpr int SR = RMCV_SR; // strip rows per workgroup
static_assert(SR == STRIP_ROWS, "the sparse kernel's frame queues assume k_binary's strip height (rmcv_internal.h)");

__device__ __forceinline__ uint32_t expand4(uint32_t nib)
{ // 4 mask bits -> 4 bytes of 0x00/0xFF
    return (((nib & 0xFu) * 0x00204081u) & 0x01010101u) * 0xFFu;
}

// 16 pixels (48 bytes in 12 dwords) -> 16-bit mask of (a - b >= lb), two pixels per packed-16 operation:
//   v_perm_b32 gathers byte a of pixels p and p+8 (24 bytes = 6 dwords apart) into the two halves of a dword (same for b),
//   t = (A + (0x8000 - lb)) - B per half: bit 15 of a half is set  <=>  a - b - lb >= 0   (|a - b - lb| < 2^15),
// the flags are collected by shifting the accumulator (bit 15 -> pixels 0..7 end in bits 8..15, bit 31 -> pixels 8..15 in bits
// 24..31) and one last v_perm picks the two bytes: 6 operations per pair of pixels.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
template <int CA, int CB>
__device__ __forceinline__ uint32_t thresh16(const uint32_t d[12], int lb)
{
    const uint32_t kk = (uint32_t)(0x8000 - lb) & 0xFFFFu;
    const uint32_t K = kk | (kk << 16);
    uint32_t acc = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int ia = 3 * j + CA, ib = 3 * j + CB; // byte offsets of pixel j; pixel j+8 is 24 bytes = 6 dwords further
        // v_perm_b32(S0, S1, sel): selector 0..3 = bytes of S1, 4..7 = bytes of S0, 0x0c = zero
        const uint32_t sa = (uint32_t)(ia & 3) | (0x0cu << 8) | ((uint32_t)((ia & 3) + 4) << 16) | (0x0cu << 24);
        const uint32_t sb = (uint32_t)(ib & 3) | (0x0cu << 8) | ((uint32_t)((ib & 3) + 4) << 16) | (0x0cu << 24);
        const uint32_t A = __builtin_amdgcn_perm(d[(ia >> 2) + 6], d[ia >> 2], sa);
        const uint32_t B = __builtin_amdgcn_perm(d[(ib >> 2) + 6], d[ib >> 2], sb);
        u16x2 t = __builtin_bit_cast(u16x2, A) + __builtin_bit_cast(u16x2, K);
        t = t - __builtin_bit_cast(u16x2, B);
        acc = (acc >> 1) | (__builtin_bit_cast(uint32_t, t) & 0x80008000u);
    }
    return __builtin_amdgcn_perm(0u, acc, 0x0c0c0301u); // byte 1 (pixels 0..7), byte 3 (pixels 8..15)
}


// The same compare through a frame's gamma table (RMCV_OPT_ENHANCE; used by k_binary_enh.hip):
// LUT[a] - LUT[b] >= lb with a non-decreasing table is a >= M[b] (enhance_math.h: enh_m_entry), so ONE lookup per pixel -- M of the
// pixel's b byte, 16 bits (0 .. 256), two of them packed into the dword thresh16 subtracts -- and the bound is folded away:
// t = (A + 0x8000) - M per half, bit 15 set  <=>  a >= M[b].  s_m: the frame's 256 entries in LDS.
template <int CA, int CB>
__device__ __forceinline__ uint32_t thresh16_m(const uint32_t d[12], const uint16_t* s_m)
{
    const uint32_t K = 0x80008000u;
    uint32_t acc = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int ia = 3 * j + CA, ib = 3 * j + CB;
        const uint32_t sa = (uint32_t)(ia & 3) | (0x0cu << 8) | ((uint32_t)((ia & 3) + 4) << 16) | (0x0cu << 24);
        const uint32_t A = __builtin_amdgcn_perm(d[(ia >> 2) + 6], d[ia >> 2], sa);
        const uint32_t b_lo = (d[ib >> 2] >> (8 * (ib & 3))) & 0xFFu, b_hi = (d[(ib >> 2) + 6] >> (8 * (ib & 3))) & 0xFFu;
        const uint32_t B = (uint32_t)s_m[b_lo] | ((uint32_t)s_m[b_hi] << 16);
        u16x2 t = __builtin_bit_cast(u16x2, A) + __builtin_bit_cast(u16x2, K);
        t = t - __builtin_bit_cast(u16x2, B);
        acc = (acc >> 1) | (__builtin_bit_cast(uint32_t, t) & 0x80008000u);
    }
    return __builtin_amdgcn_perm(0u, acc, 0x0c0c0301u);
}


// n / d for n < 2^16 with a precomputed reciprocal r = ceil(2^32 / d) (exact in that range); d == 1 gives r == 0
__device__ __forceinline__ int div_r(int n, uint32_t r) { return r ? (int)__umulhi((uint32_t)n, r) : n; }

// lb is pre-clamped on the host to [1, 256]: lb <= 0 means "everything passes" (lb = -1 flag).
// FAST (w a multiple of 64, 16-byte aligned rows, every extent below 4 GiB): the vector-memory instructions are UNCONDITIONAL
// raw-buffer operations.  A lane (or item) that has nothing to move uses an offset beyond the buffer's extent: the hardware
// answers such a load with zeros -- a row outside the image thresholds to 0 by itself -- and drops such a store.  Round 1 had
// ordinary loads behind per-lane predicates: per 16-pixel item that was ~70 instructions of EXEC save/restore, branches and
// register zeroing around the 60 that threshold (profiles/r02a_k_binary_ablations.txt: 0.14-0.18 ms of the 0.28 with the
// loads compiled out).
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2v __attribute__((ext_vector_type(2)));
typedef uint32_t u32x3v __attribute__((ext_vector_type(3)));
static constexpr uint32_t OOB = 0xFFFFFF00u; // voffset of a lane that moves nothing (extents are checked below 4 GiB - 256)
static constexpr int RSRC3 = 0x00020000;     // raw buffer descriptor word 3, gfx9 family

} // namespace rmcv
