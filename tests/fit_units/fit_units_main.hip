// TEST-ONLY stand-alone program (tests/test_gpu_fit_units.py): the scalar tails of the ellipse fit (rmcv_amd/csrc/device_fit.h,
// device_eig3.h), each alone, on the device, from one case file.  The tails are lane-resident -- their small matrices live across the
// lanes of one register -- so a case is run by one whole wavefront, the way the library's kernels run them: one workgroup of 64 threads
// per case, one launch per record, lane 0 writes the (wave-uniform) results as raw bits.
//   fit_units_main IN OUT
// IN : uint32 magic, uint32 records; per record: uint32 function id, uint32 doubles per case, uint32 result slots per case, uint32 0,
//      uint64 count, then count x (doubles per case) doubles
// OUT: uint32 magic, uint32 records; per record: uint32 function id, uint32 result slots per case, uint64 count, then count x slots
//      64-bit slots (a double's bits, or a float's / an int's in the low half)
// Built twice by the library's Makefile (target fit_units, the library's own flags): as the library compiles the eigen-solver (the
// specialised Eig3T of device_eig3.h), and with -DRMCV_EIG3_GENERAL (the run-time-subscript form it claims to equal).
// Every HIP call is checked and the first error ends the program with status 5.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../rmcv_amd/csrc/device_fit.h"

#define FIT_UNITS_MAGIC 0x54494655u /* "UFIT" */

enum { FU_EIG = 0, FU_DIRECT = 1, FU_NORMAL5 = 2, FU_NORMAL3 = 3, FU_CENTRE = 4, FU_FINISH = 5, FU_N_FUNCS = 6 };
static constexpr int fu_n_in[FU_N_FUNCS] = {9, 24, 30, 12, 5, 8};
static constexpr int fu_n_out[FU_N_FUNCS] = {12, 16, 13, 13, 2, 5};

#define HIP_OK(call)                                                                                               \
    do {                                                                                                           \
        const hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess) {                                                                                    \
            std::fprintf(stderr, "fit_units_main: %s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__);    \
            std::exit(5);                                                                                          \
        }                                                                                                          \
    } while (0)

using namespace rmcv;

__device__ __forceinline__ uint64_t bits(double v) { return (uint64_t)__double_as_longlong(v); }
__device__ __forceinline__ uint64_t bits(float v) { return (uint64_t)__float_as_uint(v); }

__device__ __forceinline__ void put_rrect(uint64_t* o, const rmcv_rrect& b)
{
    o[0] = bits(b.cx);
    o[1] = bits(b.cy);
    o[2] = bits(b.w);
    o[3] = bits(b.h);
    o[4] = bits(b.angle);
}

template <int K>
__device__ __forceinline__ void normal_unit(const double* in, uint64_t* o, int lane)
{
    LaneVec G(lane), g(lane);
    G.reg = lane < K * K ? in[lane] : 0.0;
    g.reg = lane < K ? in[K * K + lane] : 0.0;
    NormalFac F(lane);
    double wmax, wmin, x[5];
    normal_factor<K>(G, F, &wmax, &wmin);
    normal_apply<K>(F, g, x, lane);
    double lam[5];
#pragma unroll
    for (int i = 0; i < 5; i++) lam[i] = i < K ? F.lam.get(i) : 0.0;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 5; i++) o[i] = bits(lam[i]);
        o[5] = (uint64_t)(uint32_t)F.use;
        o[6] = bits(wmax);
        o[7] = bits(wmin);
#pragma unroll
        for (int i = 0; i < 5; i++) o[8 + i] = bits(x[i]);
    }
}

// one workgroup = one wavefront = one case
template <int FID>
__global__ void __launch_bounds__(64) k_fit_unit(const double* __restrict__ in_all, uint64_t* __restrict__ out_all, uint64_t count)
{
    const uint64_t c = blockIdx.x;
    if (c >= count) return;
    const int lane = threadIdx.x;
    constexpr int NI = fu_n_in[FID], NO = fu_n_out[FID];
    const double* in = in_all + c * (uint64_t)NI;
    uint64_t* o = out_all + c * (uint64_t)NO;
    if constexpr (FID == FU_EIG) {
        double M[3][3], eval[3], evec[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) M[i][j] = in[3 * i + j];
        eigen_nonsymmetric3(M, eval, evec, lane);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 3; i++) o[i] = bits(eval[i]);
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) o[3 + 3 * i + j] = bits(evec[i][j]);
        }
    } else if constexpr (FID == FU_DIRECT) {
        double DM[6][6], TM[3][3], M[3][3], Ts = 0;
        {
            int e = 0;
#pragma unroll
            for (int a = 0; a < 6; a++)
#pragma unroll
                for (int b = a; b < 6; b++, e++) DM[a][b] = DM[b][a] = in[e];
        }
        const double det = direct_reduce(DM, TM, &Ts, M);
        rmcv_rrect box = {0, 0, 0, 0, 0};
        direct_finish(M, TM, Ts, in[21], in[22], in[23], &box, lane);
        if (lane == 0) {
            o[0] = bits(det);
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) o[1 + 3 * i + j] = bits(M[i][j]);
            o[10] = bits(Ts);
            put_rrect(o + 11, box);
        }
    } else if constexpr (FID == FU_NORMAL5) {
        normal_unit<5>(in, o, lane);
    } else if constexpr (FID == FU_NORMAL3) {
        normal_unit<3>(in, o, lane);
    } else if constexpr (FID == FU_CENTRE) {
        double gfp[5], rp[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 5; i++) gfp[i] = in[i];
        general_centre(gfp, rp);
        if (lane == 0) {
            o[0] = bits(rp[0]);
            o[1] = bits(rp[1]);
        }
    } else {
        double gfp[3] = {in[0], in[1], in[2]}, rp[5] = {in[3], in[4], 0, 0, 0};
        rmcv_rrect box = {0, 0, 0, 0, 0};
        general_finish(gfp, rp, in[5], (float)in[6], (float)in[7], &box);
        if (lane == 0) put_rrect(o, box);
    }
}

static void fail(const char* what)
{
    std::fprintf(stderr, "fit_units_main: %s\n", what);
    std::exit(2);
}
static void get(std::FILE* f, void* p, size_t bytes) { if (bytes && std::fread(p, 1, bytes, f) != bytes) fail("short input"); }
static void put(std::FILE* f, const void* p, size_t bytes) { if (bytes && std::fwrite(p, 1, bytes, f) != bytes) fail("short write"); }

static void launch_unit(int fid, const double* in, uint64_t* out, uint64_t count)
{
    const dim3 grid((unsigned)count), block(64);
    switch (fid) {
        case FU_EIG: k_fit_unit<FU_EIG><<<grid, block>>>(in, out, count); break;
        case FU_DIRECT: k_fit_unit<FU_DIRECT><<<grid, block>>>(in, out, count); break;
        case FU_NORMAL5: k_fit_unit<FU_NORMAL5><<<grid, block>>>(in, out, count); break;
        case FU_NORMAL3: k_fit_unit<FU_NORMAL3><<<grid, block>>>(in, out, count); break;
        case FU_CENTRE: k_fit_unit<FU_CENTRE><<<grid, block>>>(in, out, count); break;
        case FU_FINISH: k_fit_unit<FU_FINISH><<<grid, block>>>(in, out, count); break;
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) fail("usage: fit_units_main IN OUT");
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) fail("cannot open the files");
    uint32_t head[2];
    get(in, head, sizeof(head));
    if (head[0] != FIT_UNITS_MAGIC) fail("not a case file");
    put(out, head, sizeof(head));
    for (uint32_t r = 0; r < head[1]; r++) {
        uint32_t rec[4];
        uint64_t n;
        get(in, rec, sizeof(rec));
        get(in, &n, sizeof(n));
        const int fid = (int)rec[0];
        if (fid < 0 || fid >= FU_N_FUNCS || (int)rec[1] != fu_n_in[fid] || (int)rec[2] != fu_n_out[fid] || n > (1u << 20)) fail("bad record");
        const size_t n_in = (size_t)fu_n_in[fid], n_out = (size_t)fu_n_out[fid];
        std::vector<double> a(n * n_in);
        std::vector<uint64_t> res(n * n_out);
        get(in, a.data(), a.size() * 8);
        double* d_in = nullptr;
        uint64_t* d_out = nullptr;
        HIP_OK(hipMalloc(&d_in, (a.size() ? a.size() : 1) * 8));
        HIP_OK(hipMalloc(&d_out, (res.size() ? res.size() : 1) * 8));
        HIP_OK(hipMemcpy(d_in, a.data(), a.size() * 8, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(d_out, 0xEE, (res.size() ? res.size() : 1) * 8));
        if (n) {
            launch_unit(fid, d_in, d_out, n);
            HIP_OK(hipGetLastError());
        }
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(res.data(), d_out, res.size() * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipFree(d_in));
        HIP_OK(hipFree(d_out));
        const uint32_t rec_out[2] = {rec[0], rec[2]};
        put(out, rec_out, sizeof(rec_out));
        put(out, &n, sizeof(n));
        put(out, res.data(), res.size() * 8);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) fail("short write");
    return 0;
}
