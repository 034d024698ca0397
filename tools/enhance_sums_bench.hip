// enhance_sums_bench.hip -- k_frame_sums (RMCV_OPT_ENHANCE's pass over the frames: a pure read of 3 B/px) against the bare 3:1 copy
// (3 B/px read + 1 B/px written, the copy DESIGN.md measures the pixel kernel against) in ONE process on one box, regions of the two
// alternating.  A pure read of 3 B/px moves three quarters of the copy's bytes: three quarters of the copy's measured time is the
// yardstick, the spread between the copy's own regions the margin.  The kernel is the library's (this file includes k_enhance.hip), with
// the library's flags; "tables" is the whole enqueue in front of the pixel pass (memset + sums + the table kernel).  Cold: launches
// rotate over 4 buffer sets (1-1.8 GB each: nothing stays in the 256 MB Infinity Cache).  One JSON line.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math tools/enhance_sums_bench.hip -o tools/enhance_sums_bench
//   tools/enhance_sums_bench [regions launches]
#include "../rmcv_amd/csrc/k_enhance.hip"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace rmcv;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// the grid-stride 3:1 copy of tools/membw5.hip (k31<2>): 48 bytes in, 16 bytes out per lane, non-temporal both ways
__global__ void k_copy31(const u32x4* __restrict__ in, size_t n, u32x4* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += step * 2) {
        u32x4 a[2], b[2], c[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const size_t j = i + u * step;
            if (j < n) {
                const size_t w0 = (j - lane) * 3;
                a[u] = __builtin_nontemporal_load(in + w0 + lane);
                b[u] = __builtin_nontemporal_load(in + w0 + 64 + lane);
                c[u] = __builtin_nontemporal_load(in + w0 + 128 + lane);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const size_t j = i + u * step;
            if (j < n) __builtin_nontemporal_store(a[u] ^ b[u] ^ c[u], out + j);
        }
    }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static void stats(const char* name, std::vector<double> t, double bytes)
{
    std::sort(t.begin(), t.end());
    const double med = t[t.size() / 2];
    printf("\"%s\": {\"median_ms\": %.4f, \"min_ms\": %.4f, \"max_ms\": %.4f, \"spread\": %.4f, \"tb_per_s\": %.3f}", name, med, t.front(), t.back(),
           (t.back() - t.front()) / med, bytes / med / 1e9);
}

int main(int argc, char** argv)
{
    const int regions = argc > 1 ? atoi(argv[1]) : 7, K = argc > 2 ? atoi(argv[2]) : 20;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int geoms[2][3] = {{256, 1280, 1024}, {256, 1920, 1200}};
    printf("{\"tool\": \"enhance_sums_bench\", \"device\": \"%s\", \"cus\": %d, \"regions\": %d, \"launches_per_region\": %d", prop.gcnArchName, prop.multiProcessorCount,
           regions, K);
    for (const auto& gm : geoms) {
        const int n = gm[0], w = gm[1], h = gm[2];
        const size_t px = (size_t)n * w * h, in_bytes = 3 * px, out_bytes = px;
        constexpr int SETS = 4;
        uint8_t *in[SETS], *out[SETS];
        for (int s = 0; s < SETS; s++) {
            CK(hipMalloc((void**)&in[s], in_bytes));
            CK(hipMalloc((void**)&out[s], out_bytes));
            CK(hipMemset(in[s], 37 + s, in_bytes));
        }
        Geom g{};
        g.device = 0; g.n_cu = prop.multiProcessorCount; g.n_frames = n; g.w = w; g.h = h; g.stride = 3 * w; g.frame_pitch = (int64_t)3 * w * h;
        g.enh_max_gain = 100.0f; g.enh_min_gain = 50.0f;
        Bufs b{};
        CK(hipMalloc((void**)&b.enh_sums, (size_t)n * 24));
        CK(hipMalloc((void**)&b.enh_gamma, (size_t)n * 4));
        CK(hipMalloc((void**)&b.enh_lut, (size_t)n * 256));
        CK(hipMalloc((void**)&b.enh_m, (size_t)n * 512));
        const int strips = (h + SUM_ROWS - 1) / SUM_ROWS, n_units = n * strips;
        const int grid = std::min(g.n_cu * 8, ((n_units + g.n_cu - 1) / g.n_cu) * g.n_cu);
        int rot = 0;
        auto region = [&](int which) -> double {
            if (hipDeviceSynchronize() != hipSuccess) return -1;
            const auto t0 = std::chrono::steady_clock::now();
            for (int i = 0; i < K; i++) {
                const int s = rot++ % SETS;
                if (which == 0) hipLaunchKernelGGL(k_copy31, dim3(768), dim3(256), 0, 0, (const u32x4*)in[s], out_bytes / 16, (u32x4*)out[s]);
                else if (which == 1)
                    (void)launch(k_frame_sums<1>, dim3(grid), dim3(256), 0, nullptr, (const uint8_t*)in[s], g.frame_pitch, g.stride, n, w, h, strips, n_units,
                                 reinterpret_cast<unsigned long long*>(b.enh_sums));
                else {
                    b.frames = in[s];
                    (void)launch_enhance_tables(g, b, 80, nullptr);
                }
            }
            if (hipDeviceSynchronize() != hipSuccess) return -1;
            return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / K;
        };
        for (int which = 0; which < 3; which++) region(which); // warm-up
        std::vector<double> t[3];
        for (int r = 0; r < regions; r++)
            for (int q = 0; q < 3; q++) {
                const int which = (q + r) % 3; // none always behind the same neighbour
                const double ms = region(which);
                if (ms < 0) { fprintf(stderr, "a launch failed: %s\n", hipGetErrorString(hipGetLastError())); return 1; }
                t[which].push_back(ms);
            }
        // the sums of the constant-filled buffers, as a check that the kernel read everything: every byte of set s is 37 + s
        std::vector<unsigned long long> hs(3);
        CK(hipMemset(b.enh_sums, 0, 24));
        (void)launch(k_frame_sums<1>, dim3(grid), dim3(256), 0, nullptr, (const uint8_t*)in[1], g.frame_pitch, g.stride, n, w, h, strips, n_units,
                     reinterpret_cast<unsigned long long*>(b.enh_sums));
        CK(hipMemcpy(hs.data(), b.enh_sums, 24, hipMemcpyDeviceToHost));
        const bool ok = hs[0] == 38ull * w * h && hs[1] == hs[0] && hs[2] == hs[0];
        printf(", \"%dx%dx%d\": {\"sums_exact\": %s, ", n, w, h, ok ? "true" : "false");
        stats("copy31", t[0], (double)in_bytes + out_bytes);
        printf(", ");
        stats("k_frame_sums", t[1], (double)in_bytes);
        printf(", ");
        stats("tables", t[2], (double)in_bytes);
        std::vector<double> c0 = t[0], c1 = t[1];
        std::sort(c0.begin(), c0.end());
        std::sort(c1.begin(), c1.end());
        printf(", \"yardstick_ms\": %.4f, \"sums_over_yardstick\": %.3f}", 0.75 * c0[c0.size() / 2], c1[c1.size() / 2] / (0.75 * c0[c0.size() / 2]));
        for (int s = 0; s < SETS; s++) { (void)hipFree(in[s]); (void)hipFree(out[s]); }
        (void)hipFree(b.enh_sums); (void)hipFree(b.enh_gamma); (void)hipFree(b.enh_lut); (void)hipFree(b.enh_m);
    }
    printf("}\n");
    return 0;
}
