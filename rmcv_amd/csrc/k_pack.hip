// k_pack.hip -- the session recorder's lossless frame packer on the device (the format and the per-segment rule:
// device_pack.h, the same source rmcv_pack_host runs on the CPU).
//
// Mapping (gfx950, wave64).  A segment is 256 bytes = 64 lanes x one dword; lane L holds the row's bytes 4 L .. 4 L + 3 of the segment.
//   k_pack_widths   one wavefront per row (four rows a workgroup), walking the row's segments.  A lane's predecessors come from its own
//                   dword and its left neighbour's (__shfl_up; lane 0 takes the last dword of the segment before, carried in a
//                   register).  The OR of the raw bytes and of the zigzagged differences is reduced over the wave (6 x __shfl_xor on one
//                   packed value): its bit lengths are b_raw and b_pred.  Writes the row's header bytes and its payload size (row table).
//   k_pack_scan     one workgroup per frame: the exclusive scan of the row sizes in place (256 rows a step, wave scans + 4 partials in
//                   LDS), entry h and the frame's packed size, the zero padding, and -- for the recorder -- the frame's effective
//                   detection key and window origin copied alongside.
//   k_pack_emit     one wavefront per row again: the row's offset from the table, the segments' widths from the header, and per segment
//                   4 b ballots: word (j, k) = __ballot(bit j of the lane's coded byte k).  The wave-uniform words are handed to lanes
//                   0 .. 4 b - 1, which store them as one run of u64 -- ordinary vector stores, 32 b contiguous bytes.
//   k_unpack        one wavefront (a 64-thread workgroup) per row, walking its segments: 4 b words in, each lane gathers its four coded
//                   bytes from bit `lane` of the words; a predicted segment's differences become values by a strided running sum in LDS
//                   (260 bytes: the last dword of the segment before, then the segment; steps lag, 2 lag, 4 lag ... < 260).
// Three launches to pack: no workgroup waits for another inside a launch; every loop is bounded by h, S or b.  Nothing is indexed dynamically
// in registers (no scratch).  The frames are read twice (widths, emit); the second read comes from L2 / MALL for frames that fit.
#include "rmcv_internal.h"
#include "device_pack.h"

namespace rmcv {

// the row's bytes i0 .. i0 + 3 as a dword, bytes at or beyond w_bytes as 0 and never read; al: the row starts on a 4-byte boundary
__device__ inline uint32_t pack_load4(const uint8_t* __restrict__ row, int i0, int w_bytes, bool al)
{
    if (i0 + 3 < w_bytes) {
        if (al) return *reinterpret_cast<const uint32_t*>(row + i0);
        return (uint32_t)row[i0] | (uint32_t)row[i0 + 1] << 8 | (uint32_t)row[i0 + 2] << 16 | (uint32_t)row[i0 + 3] << 24;
    }
    uint32_t v = 0;
    for (int k = 0; k < 3; k++)
        if (i0 + k < w_bytes) v |= (uint32_t)row[i0 + k] << (8 * k);
    return v;
}

// the zigzagged differences of the lane's four bytes (cur) to the bytes `lag` before them (prev: the dword to the left), virtual bytes 0
__device__ inline uint32_t pack_residuals(uint32_t cur, uint32_t prev, int lag, int i0, int w_bytes)
{
    const uint64_t win = (uint64_t)cur << 32 | prev;
    uint32_t zz = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned v = (cur >> (8 * k)) & 0xFFu, pred = (unsigned)(win >> (8 * (4 + k - lag))) & 0xFFu;
        const unsigned z = i0 + k < w_bytes ? pack_zigzag((v - pred) & 0xFFu) : 0u;
        zz |= z << (8 * k);
    }
    return zz;
}

// the plane a workgroup's frame index names
__device__ inline const uint8_t* pack_plane(const PackJob& j, int f) { return j.frames + (int64_t)(j.use_idx ? j.idx.f[f] : f) * j.pitch; }

__global__ __launch_bounds__(256) void k_pack_widths(PackJob j)
{
    const int lane = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6), f = blockIdx.y;
    if (y >= j.h) return; // (no barrier below: a wavefront is on its own)
    const int S = pack_segments(j.w_bytes);
    const uint8_t* row = pack_plane(j, f) + (int64_t)y * j.stride;
    const bool al = ((uintptr_t)row & 3) == 0;
    uint8_t* out = j.out + (int64_t)f * j.out_pitch;
    uint32_t* tab = reinterpret_cast<uint32_t*>(out + pack_header_bytes(j.w_bytes, j.h));
    uint32_t carry = 0, total = 0, hb_mine = 0;
    for (int s = 0; s < S; s++) {
        const int i0 = s * PACK_SEG + 4 * lane;
        const uint32_t cur = pack_load4(row, i0, j.w_bytes, al);
        uint32_t prev = (uint32_t)__shfl_up((int)cur, 1);
        if (lane == 0) prev = carry;
        const uint32_t zz = pack_residuals(cur, prev, j.lag, i0, j.w_bytes);
        carry = (uint32_t)__shfl((int)cur, 63);
        uint32_t o = ((cur | cur >> 8 | cur >> 16 | cur >> 24) & 0xFFu) | ((zz | zz >> 8 | zz >> 16 | zz >> 24) & 0xFFu) << 8;
#pragma unroll
        for (int d = 32; d; d >>= 1) o |= (uint32_t)__shfl_xor((int)o, d);
        const uint32_t hb = pack_header(pack_bitlen(o & 0xFFu), pack_bitlen(o >> 8));
        total += 32 * (hb & 15u);
        if (lane == (s & 63)) hb_mine = hb;
        if ((s & 63) == 63 || s == S - 1) { // the header bytes of up to 64 segments leave together
            if (lane <= (s & 63)) out[(int64_t)y * S + (s & ~63) + lane] = (uint8_t)hb_mine;
        }
    }
    if (lane == 0) tab[y] = total;
}

__global__ __launch_bounds__(256) void k_pack_scan(PackJob j)
{
    __shared__ uint32_t s_part[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, f = blockIdx.x;
    const int S = pack_segments(j.w_bytes);
    const int64_t H = pack_header_bytes(j.w_bytes, j.h), T = pack_table_bytes(j.h);
    uint8_t* out = j.out + (int64_t)f * j.out_pitch;
    uint32_t* tab = reinterpret_cast<uint32_t*>(out + H);
    uint32_t before = 0;
    for (int base = 0; base < j.h; base += 256) {
        const int y = base + tid;
        const uint32_t v = y < j.h ? tab[y] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)incl, d);
            if (lane >= d) incl += t;
        }
        if (lane == 63) s_part[wv] = incl;
        __syncthreads();
        uint32_t left = 0, all = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k < wv) left += s_part[k];
            all += s_part[k];
        }
        if (y < j.h) tab[y] = before + left + incl - v;
        before += all;
        __syncthreads();
    }
    for (int64_t i = (int64_t)j.h * S + tid; i < H; i += 256) out[i] = 0;
    if (tid == 0) {
        tab[j.h] = before;
        if (4 * ((int64_t)j.h + 1) < T) tab[j.h + 1] = 0;
        j.sizes[f] = H + T + (int64_t)before;
        const int src = j.use_idx ? j.idx.f[f] : f;
        if (j.keys_out) {
            const FrameKey k = j.key_eff[src];
            memcpy(j.keys_out + 4 * f, &k, sizeof(k));
            j.camps_out[f] = j.key_enemy[src];
        }
        if (j.origins_out) j.origins_out[f] = j.win_eff[src];
    }
}

__global__ __launch_bounds__(256) void k_pack_emit(PackJob j)
{
    const int lane = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6), f = blockIdx.y;
    if (y >= j.h) return;
    const int S = pack_segments(j.w_bytes);
    const uint8_t* row = pack_plane(j, f) + (int64_t)y * j.stride;
    const bool al = ((uintptr_t)row & 3) == 0;
    uint8_t* out = j.out + (int64_t)f * j.out_pitch;
    const int64_t H = pack_header_bytes(j.w_bytes, j.h);
    const uint32_t* tab = reinterpret_cast<const uint32_t*>(out + H);
    uint64_t* dst = reinterpret_cast<uint64_t*>(out + H + pack_table_bytes(j.h) + tab[y]);
    uint32_t carry = 0;
    for (int s = 0; s < S; s++) {
        const int i0 = s * PACK_SEG + 4 * lane;
        const uint32_t cur = pack_load4(row, i0, j.w_bytes, al);
        uint32_t prev = (uint32_t)__shfl_up((int)cur, 1);
        if (lane == 0) prev = carry;
        carry = (uint32_t)__shfl((int)cur, 63);
        const uint32_t hb = (uint32_t)__builtin_amdgcn_readfirstlane((int)out[(int64_t)y * S + s]);
        const int b = (int)(hb & 15u);
        if (b == 0) continue;
        const uint32_t coded = (hb & PACK_MODE_PRED) ? pack_residuals(cur, prev, j.lag, i0, j.w_bytes) : cur;
        uint64_t mine = 0;
        for (int jb = 0; jb < b; jb++) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint64_t word = __ballot((coded >> (8 * k + jb)) & 1u);
                if (lane == 4 * jb + k) mine = word;
            }
        }
        if (lane < 4 * b) dst[lane] = mine;
        dst += 4 * b;
    }
}

// per-byte sum mod 256 of two packed dwords
__device__ inline uint32_t pack_add4(uint32_t a, uint32_t b) { return ((a & 0x7F7F7F7Fu) + (b & 0x7F7F7F7Fu)) ^ ((a ^ b) & 0x80808080u); }

struct UnpackJob {
    const uint8_t* packed;
    int64_t in_pitch;
    int w_bytes, h, lag;
    uint8_t* frames;
    int stride;
    int64_t pitch;
};

__global__ __launch_bounds__(64) void k_unpack(UnpackJob j)
{
    __shared__ uint32_t s_x[65]; // [0]: the last dword of the segment before (only its last `lag` bytes kept); [1 + L]: lane L's dword
    const int lane = threadIdx.x, y = blockIdx.x, f = blockIdx.y;
    const int S = pack_segments(j.w_bytes);
    const int64_t H = pack_header_bytes(j.w_bytes, j.h), T = pack_table_bytes(j.h);
    const uint8_t* in = j.packed + (int64_t)f * j.in_pitch;
    const int64_t room = j.in_pitch - H - T; // bytes of the frame's payload area at most
    int64_t off = (int64_t)__builtin_amdgcn_readfirstlane((int)reinterpret_cast<const uint32_t*>(in + H)[y]) & 0xFFFFFFFFll;
    if (off & 7) return; // (no packer writes such an offset: an inconsistent buffer is left unfinished, never read past its area)
    uint8_t* row = j.frames + (int64_t)f * j.pitch + (int64_t)y * j.stride;
    const bool al = ((uintptr_t)row & 3) == 0;
    const uint32_t keep = j.lag == 4 ? ~0u : ~0u << (8 * (4 - j.lag));
    const uint8_t* s_b = reinterpret_cast<const uint8_t*>(s_x);
    uint32_t carry = 0;
    for (int s = 0; s < S; s++) {
        const uint32_t hb = (uint32_t)__builtin_amdgcn_readfirstlane((int)in[(int64_t)y * S + s]);
        const int b = (int)(hb & 15u) > 8 ? 8 : (int)(hb & 15u);
        if (off + 32 * b > room) return;
        const uint64_t* src = reinterpret_cast<const uint64_t*>(in + H + T + off);
        off += 32 * b;
        const uint64_t mine = lane < 4 * b ? src[lane] : 0ull;
        const uint32_t lo = (uint32_t)mine, hi = (uint32_t)(mine >> 32);
        uint32_t coded = 0;
        for (int jb = 0; jb < b; jb++) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t wlo = (uint32_t)__shfl((int)lo, 4 * jb + k), whi = (uint32_t)__shfl((int)hi, 4 * jb + k); // word 4 jb + k, for every lane
                const uint32_t bit = ((lane < 32 ? wlo : whi) >> (lane & 31)) & 1u;
                coded |= bit << (8 * k + jb);
            }
        }
        uint32_t v = coded;
        if (hb & PACK_MODE_PRED) {
            uint32_t x = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) x |= pack_unzigzag((coded >> (8 * k)) & 0xFFu) << (8 * k);
            s_x[1 + lane] = x;
            if (lane == 0) s_x[0] = carry & keep;
            __syncthreads();
            for (int d = j.lag; d < PACK_SEG + 4; d <<= 1) {
                uint32_t add = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int at = 4 + 4 * lane + k - d;
                    if (at >= 0) add |= (uint32_t)s_b[at] << (8 * k);
                }
                __syncthreads();
                x = pack_add4(x, add);
                s_x[1 + lane] = x;
                __syncthreads();
            }
            v = x;
        }
        carry = (uint32_t)__shfl((int)v, 63);
        const int i0 = s * PACK_SEG + 4 * lane;
        if (i0 + 3 < j.w_bytes && al) *reinterpret_cast<uint32_t*>(row + i0) = v;
        else
            for (int k = 0; k < 4; k++)
                if (i0 + k < j.w_bytes) row[i0 + k] = (uint8_t)(v >> (8 * k));
    }
}

const char* pack_job_refusal(const void* frames, int n, int w_bytes, int h, int stride, int64_t pitch, int lag, const void* packed, int64_t packed_pitch)
{
    if (!frames || !packed) return "null frames or packed buffer";
    if (n < 1 || n > 65535) return "n out of range (1 .. 65535)";
    if (!pack_geometry_ok(w_bytes, h, lag)) return "w_bytes, h >= 1, lag 1 .. 4, and a payload below 2^31 bytes";
    if (stride < w_bytes) return "stride < w_bytes";
    if (n > 1 && pitch < (int64_t)stride * (h - 1) + w_bytes) return "frame pitch smaller than a frame";
    if (((uintptr_t)packed | (uintptr_t)packed_pitch) & 7) return "the packed buffer and its pitch must be multiples of 8";
    if (packed_pitch < pack_header_bytes(w_bytes, h) + pack_table_bytes(h)) return "packed pitch smaller than a packed frame's header and row table";
    return nullptr;
}

hipError_t launch_pack(const PackJob& j, hipStream_t s)
{
    const dim3 rows((j.h + 3) / 4, j.n);
    hipError_t e = launch(k_pack_widths, rows, dim3(256), 0, s, j);
    if (e == hipSuccess) e = launch(k_pack_scan, dim3(j.n), dim3(256), 0, s, j);
    if (e == hipSuccess) e = launch(k_pack_emit, rows, dim3(256), 0, s, j);
    return e;
}

hipError_t launch_unpack(const uint8_t* packed, int64_t in_pitch, int n, int w_bytes, int h, int lag, uint8_t* frames, int stride, int64_t pitch, hipStream_t s)
{
    const UnpackJob j{packed, in_pitch, w_bytes, h, lag, frames, stride, pitch};
    return launch(k_unpack, dim3(h, n), dim3(64), 0, s, j);
}

} // namespace rmcv

using namespace rmcv;

extern "C" {

int64_t rmcv_pack_bound(int w_bytes, int h) { return pack_geometry_ok(w_bytes, h, 1) ? pack_bound(w_bytes, h) : (int64_t)RMCV_ERR_BAD_ARG; }

int rmcv_pack_host(const uint8_t* src, int w_bytes, int h, int64_t stride, int lag, uint8_t* out, int64_t cap, int64_t* size)
{
    return pack_host(src, w_bytes, h, stride, lag, out, cap, size);
}

int rmcv_unpack_host(const uint8_t* packed, int64_t len, int w_bytes, int h, int lag, uint8_t* dst, int64_t stride)
{
    return unpack_host(packed, len, w_bytes, h, lag, dst, stride);
}

int rmcv_pack_frames(int device, const void* d_frames, int n, int w_bytes, int h, int stride, int64_t pitch, int lag, void* d_out, int64_t out_pitch,
                     int64_t* d_sizes, void* hip_stream)
{
    if (!d_sizes || pack_job_refusal(d_frames, n, w_bytes, h, stride, pitch, lag, d_out, out_pitch)) return RMCV_ERR_BAD_ARG;
    if (out_pitch < pack_bound(w_bytes, h)) return RMCV_ERR_BAD_ARG;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return RMCV_ERR_NO_DEVICE; }
    PackJob j{};
    j.frames = (const uint8_t*)d_frames, j.pitch = pitch, j.stride = stride, j.w_bytes = w_bytes, j.h = h, j.lag = lag, j.n = n;
    j.out = (uint8_t*)d_out, j.out_pitch = out_pitch, j.sizes = d_sizes;
    if (launch_pack(j, (hipStream_t)hip_stream) != hipSuccess) { (void)hipGetLastError(); return RMCV_ERR_HIP; }
    return RMCV_OK;
}

int rmcv_unpack_frames(int device, const void* d_packed, int n, int w_bytes, int h, int64_t in_pitch, int lag, void* d_frames, int stride,
                       int64_t pitch, void* hip_stream)
{
    if (pack_job_refusal(d_frames, n, w_bytes, h, stride, pitch, lag, d_packed, in_pitch)) return RMCV_ERR_BAD_ARG;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return RMCV_ERR_NO_DEVICE; }
    if (launch_unpack((const uint8_t*)d_packed, in_pitch, n, w_bytes, h, lag, (uint8_t*)d_frames, stride, pitch, (hipStream_t)hip_stream) != hipSuccess) {
        (void)hipGetLastError();
        return RMCV_ERR_HIP;
    }
    return RMCV_OK;
}

} // extern "C"
