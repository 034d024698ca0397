// TEST-ONLY stand-alone program (tests/test_leaf_cpu.py, tests/test_gpu_leaf.py): every leaf function of pinned_math.h and enhance_math.h,
// evaluated on the device and by this file's own host pass (hipcc's clang), from one case file.
//   leaf_main [--host-only] IN OUT
// IN : uint32 magic, uint32 records; per record: uint32 function id, uint32 element type (kept for the reader: the id decides), uint32 argument
//      arrays, uint32 0, uint64 count, then the argument arrays, `count` 64-bit slots each (tests/leaf/leaf_funcs.h says what a slot holds)
// OUT: uint32 magic, uint32 records, uint32 has_device, uint32 0; per record: uint32 function id, uint32 0, uint64 count, the device's results
//      (`count` slots; left out under --host-only), the host loop's results (`count` slots)
// The kernel is as plain as a kernel gets: one element per thread, grid-stride, 256 threads per block, no LDS.  Under --host-only no HIP call
// is made at all.  Every HIP call is checked and the first error ends the program with status 5.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "leaf_funcs.h"

#define HIP_OK(call)                                                                                          \
    do {                                                                                                      \
        const hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) {                                                                               \
            std::fprintf(stderr, "leaf_main: %s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__);    \
            std::exit(5);                                                                                     \
        }                                                                                                     \
    } while (0)

struct LeafArgs {
    const uint64_t* a[LEAF_MAX_ARGS];
};

template <int FID> __global__ void __launch_bounds__(256) k_leaf(LeafArgs args, uint64_t* out, uint64_t n)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) out[i] = leaf_eval(FID, args.a, i);
}

#define LEAF_ALL(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) X(21) \
    X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)
static_assert(LEAF_N_FUNCS == 33, "LEAF_ALL lists every id");

static void launch(int fid, const LeafArgs& args, uint64_t* out, uint64_t n)
{
    const unsigned blocks = (unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    switch (fid) {
#define X(id) case id: k_leaf<id><<<blocks, 256>>>(args, out, n); break;
        LEAF_ALL(X)
#undef X
    }
}

static void fail(const char* what)
{
    std::fprintf(stderr, "leaf_main: %s\n", what);
    std::exit(2);
}
static void get(std::FILE* f, void* p, size_t bytes) { if (bytes && std::fread(p, 1, bytes, f) != bytes) fail("short input"); }
static void put(std::FILE* f, const void* p, size_t bytes) { if (bytes && std::fwrite(p, 1, bytes, f) != bytes) fail("short write"); }

int main(int argc, char** argv)
{
    static const int nargs_of[LEAF_N_FUNCS] = LEAF_NARGS_TABLE;
    const bool host_only = argc == 4 && std::strcmp(argv[1], "--host-only") == 0;
    if (!(argc == 3 || host_only)) fail("usage: leaf_main [--host-only] IN OUT");
    std::FILE* in = std::fopen(argv[argc - 2], "rb");
    std::FILE* out = std::fopen(argv[argc - 1], "wb");
    if (!in || !out) fail("cannot open the files");
    uint32_t head[2];
    get(in, head, sizeof(head));
    if (head[0] != LEAF_MAGIC) fail("not a case file");
    const uint32_t out_head[4] = {LEAF_MAGIC, head[1], host_only ? 0u : 1u, 0u};
    put(out, out_head, sizeof(out_head));
    for (uint32_t r = 0; r < head[1]; r++) {
        uint32_t rec[4];
        uint64_t n;
        get(in, rec, sizeof(rec));
        get(in, &n, sizeof(n));
        const int fid = (int)rec[0];
        if (fid < 0 || fid >= LEAF_N_FUNCS || (int)rec[2] != nargs_of[fid] || n > (1u << 22)) fail("bad record");
        std::vector<std::vector<uint64_t>> a(rec[2], std::vector<uint64_t>(n));
        const uint64_t* ptr[LEAF_MAX_ARGS] = {};
        for (uint32_t k = 0; k < rec[2]; k++) {
            get(in, a[k].data(), n * 8);
            ptr[k] = a[k].data();
        }
        std::vector<uint64_t> res(n);
        const uint32_t rec_out[2] = {rec[0], 0u};
        put(out, rec_out, sizeof(rec_out));
        put(out, &n, sizeof(n));
        if (!host_only) {
            LeafArgs d = {};
            uint64_t* d_out = nullptr;
            for (uint32_t k = 0; k < rec[2]; k++) {
                uint64_t* p = nullptr;
                HIP_OK(hipMalloc(&p, (n ? n : 1) * 8));
                HIP_OK(hipMemcpy(p, a[k].data(), n * 8, hipMemcpyHostToDevice));
                d.a[k] = p;
            }
            HIP_OK(hipMalloc(&d_out, (n ? n : 1) * 8));
            HIP_OK(hipMemset(d_out, 0xEE, (n ? n : 1) * 8));
            if (n) {
                launch(fid, d, d_out, n);
                HIP_OK(hipGetLastError());
            }
            HIP_OK(hipDeviceSynchronize());
            HIP_OK(hipMemcpy(res.data(), d_out, n * 8, hipMemcpyDeviceToHost));
            for (uint32_t k = 0; k < rec[2]; k++) HIP_OK(hipFree(const_cast<uint64_t*>(d.a[k])));
            HIP_OK(hipFree(d_out));
            put(out, res.data(), n * 8);
        }
        for (uint64_t i = 0; i < n; i++) res[i] = leaf_eval(fid, ptr, i);
        put(out, res.data(), n * 8);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) fail("short write");
    return 0;
}
