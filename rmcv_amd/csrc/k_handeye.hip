// k_handeye.hip -- the hand-eye solve: calibrateHandEye of executable/calibration/hand_eye.cpp:140-155 and its check loop
// (:157-180) on the view table the calibration solve left on the device and a table of gimbal attitudes, a whole fleet in one launch.  The
// arithmetic is device_handeye.h, the same source rmcv_calibrate_hand_eye_host runs on the CPU; what is decided outside the kernel is
// handeye_plan.h.
//
// Mapping (gfx950, wave64).  k_handeye: one workgroup of four wavefronts per camera, the whole solve inside the launch.  Wavefront 0 compacts
// the camera's used views into an ascending list (one lane per view: ballot and popcount); thread u stages used view u -- the gimbal's
// matrix and quaternion, the board's pose, 23 doubles -- into LDS, so a view is read from HBM once although it takes part in up to 255
// pairs; the pairs are dealt over the 256 threads, thread T walking pairs T, T + 256, .. without a division (handeye_pair_advance); each
// pass over the pairs ends in butterflies of __shfl_xor on doubles and one add across the wavefronts through LDS.  The 4 x 4 Jacobi runs on
// wavefront 0 with lane r on row r of each rotation, one thread factors the 3 x 3, and two passes over the views and one over the pairs
// give the check loop and the residuals.  Ordinary vector loads and stores; no atomics, no workspace, no scratch.
#include "rmcv_internal.h"
#include "device_handeye.h"

namespace rmcv {

// who runs what on the device: device_handeye.h's HandEyeHostExec is the same, one after the other
struct HandEyeDevExec {
    double* red;   // [HANDEYE_WAVES][HANDEYE_SUMS_MAX] the wavefronts' results of a sum
    int tid, lane, wave;
    __device__ __forceinline__ void wave_sync()
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    template <int N>
    __device__ __forceinline__ void reduce(double* acc, double* out)
    {
        static_assert(N <= HANDEYE_SUMS_MAX, "a sum's partials fit the LDS set aside for them");
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
            for (int n = 0; n < N; n++) acc[n] = acc[n] + __shfl_xor(acc[n], s);
        }
        if (lane == 0) {
#pragma unroll
            for (int n = 0; n < N; n++) red[wave * HANDEYE_SUMS_MAX + n] = acc[n];
        }
        __syncthreads();
#pragma unroll
        for (int n = 0; n < N; n++)
            out[n] = ((red[n] + red[HANDEYE_SUMS_MAX + n]) + red[2 * HANDEYE_SUMS_MAX + n]) + red[3 * HANDEYE_SUMS_MAX + n];
        __syncthreads();
    }
    template <int N, class F>
    __device__ __forceinline__ void pair_sum(int n, F f, double* out)
    {
        double acc[N];
#pragma unroll
        for (int k = 0; k < N; k++) acc[k] = 0.0;
        int i = 0, j = 1;
        handeye_pair_advance(i, j, tid, n);
        while (i < n - 1) {
            f(i, j, acc);
            handeye_pair_advance(i, j, HANDEYE_THREADS, n);
        }
        reduce<N>(acc, out);
    }
    template <int N, class F>
    __device__ __forceinline__ void view_sum(int n, F f, double* out)
    {
        double acc[N];
#pragma unroll
        for (int k = 0; k < N; k++) acc[k] = 0.0;
        for (int u = tid; u < n; u += HANDEYE_THREADS) f(u, acc);
        reduce<N>(acc, out);
    }
    template <class F>
    __device__ __forceinline__ void lanes(int n, F f)
    {
        wave_sync();
        if (lane < n) f(lane);
        wave_sync();
    }
    template <class F>
    __device__ __forceinline__ void wave0(F f)
    {
        __syncthreads();
        if (wave == 0) f();
        __syncthreads();
    }
    template <class F>
    __device__ __forceinline__ void each(int n, F f)
    {
        __syncthreads();
        for (int i = tid; i < n; i += HANDEYE_THREADS) f(i);
        __syncthreads();
    }
};
static_assert(HANDEYE_WAVES == 4, "reduce adds four wavefronts' results");

__global__ __launch_bounds__(HANDEYE_THREADS) void k_handeye(HandEyeJob j)
{
    __shared__ double s_stage[CALIB_VIEWS_PER_CAMERA_MAX * HANDEYE_VIEW_LDS];
    __shared__ double s_red[HANDEYE_WAVES * HANDEYE_SUMS_MAX];
    __shared__ HandEyeCam s_cam;
    __shared__ int32_t s_list[CALIB_VIEWS_PER_CAMERA_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, cam = blockIdx.x;
    if (wv == 0) {   // the camera's used views in ascending order
        int n = 0;
        for (int base = 0; base < j.n_views; base += 64) {
            const int v = base + lane;
            const bool in = v < j.n_views && handeye_view_used(j, v, cam);
            const uint64_t m = __ballot(in);
            const int at = n + __popcll(m & ((1ull << lane) - 1));
            if (in && at < CALIB_VIEWS_PER_CAMERA_MAX) s_list[at] = v;
            n += __popcll(m);
        }
        if (lane == 0) s_cam.nused = n;
    }
    __syncthreads();
    HandEyeDevExec x{s_red, tid, lane, wv};
    handeye_camera(x, s_cam, s_list, s_stage, j, cam);
}

hipError_t launch_handeye(const HandEyeJob& j, hipStream_t s)
{
    return launch(k_handeye, dim3((unsigned)handeye_workgroups(j.n_cameras)), dim3(HANDEYE_THREADS), 0, s, j);
}

} // namespace rmcv
