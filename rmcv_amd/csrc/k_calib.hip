// k_calib.hip -- the calibration solve: calibrateCamera of executable/calibration/hand_eye.cpp:128-131 on the corner tables
// find and refine left on the device, a whole fleet in one call.  The arithmetic is device_calib.h, the same source
// rmcv_calibrate_camera_host runs on the CPU; what is decided outside the kernels is calib_plan.h.
//
// Mapping (gfx950, wave64).  k_calib_homography: one wavefront per view, four per workgroup: the view's flag (count and finiteness, a ballot),
// Hartley's sums and the 45 sums of A^T A as butterflies of __shfl_xor on doubles, the 9 x 9 Jacobi in the wavefront's LDS with lane r on row
// r of each rotation.  k_calib_solve: one workgroup of four wavefronts per camera; wavefront 0 compacts the camera's used views into an
// ascending list (ballot and popcount); then the whole Levenberg-Marquardt loop runs inside the launch: the wavefronts take the views in
// turn -- the inner loop, residual and Jacobian per point, feeds the 136 per-view sums in five passes of at most 33 doubles per lane, each
// pass recomputing the Jacobian, into the wavefront's LDS; lanes 0 .. 53 eliminate the view's pose block -- and between them one thread per
// matrix entry walks the views in ascending order for the cross-view sums.  Ordinary vector loads and stores; no scratch.
#include "rmcv_internal.h"
#include "device_calib.h"

namespace rmcv {

// who runs what on the device: device_calib.h's CalibHostExec is the same, one after the other
template <int WAVES>
struct CalibDevExec {
    double* lds;   // this wavefront's
    int tid, lane, wave;
    __device__ __forceinline__ void wave_sync()
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    template <int N, class F>
    __device__ __forceinline__ void wsum(int P, F f, double* out)
    {
        double acc[N];
#pragma unroll
        for (int n = 0; n < N; n++) acc[n] = 0.0;
        for (int k = lane; k < P; k += 64) f(k, acc);
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
            for (int n = 0; n < N; n++) acc[n] = acc[n] + __shfl_xor(acc[n], s);
        }
#pragma unroll
        for (int n = 0; n < N; n++) out[n] = acc[n];
    }
    __device__ __forceinline__ double* wave_lds() { return lds; }
    template <class F>
    __device__ __forceinline__ void lanes(int n, F f)
    {
        wave_sync();
        if (lane < n) f(lane);
        wave_sync();
    }
    template <class F>
    __device__ __forceinline__ void each_view(int n, F f)
    {
        __syncthreads();
        for (int i = wave; i < n; i += WAVES) f(i);
        __syncthreads();
    }
    template <class F>
    __device__ __forceinline__ void each(int n, F f)
    {
        __syncthreads();
        for (int i = tid; i < n; i += 64 * WAVES) f(i);
        __syncthreads();
    }
};

__global__ __launch_bounds__(64 * CALIB_HOMOGRAPHY_WAVES) void k_calib_homography(CalibJob j)
{
    __shared__ double s_lds[CALIB_HOMOGRAPHY_WAVES][CALIB_WAVE_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int v = blockIdx.x * CALIB_HOMOGRAPHY_WAVES + wv;
    if (v >= j.n_views) return;   // (no workgroup barrier in this kernel)
    const int P = j.cols * j.rows;
    const bool mine = calib_points_finite(j.corners + (int64_t)v * j.per_frame * 2, P, lane, 64);
    const bool used = j.counts[v] == P && __all(mine);
    if (lane == 0) j.vcam[v] = used ? frame_camera_eff(j.view_camera ? j.view_camera[v] : 0, j.n_cameras) : -1;
    if (!used) return;
    CalibDevExec<CALIB_HOMOGRAPHY_WAVES> x{s_lds[wv], tid, lane, wv};
    calib_view_homography(x, j, v);
}

__global__ __launch_bounds__(64 * CALIB_SOLVE_WAVES) void k_calib_solve(CalibJob j)
{
    __shared__ double s_lds[CALIB_SOLVE_WAVES][CALIB_WAVE_LDS];
    __shared__ CalibCam s_cam;
    __shared__ int32_t s_list[CALIB_VIEWS_PER_CAMERA_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, cam = blockIdx.x;
    if (wv == 0) {   // the camera's used views in ascending order
        int n = 0;
        for (int base = 0; base < j.n_views; base += 64) {
            const int v = base + lane;
            const bool in = v < j.n_views && j.vcam[v] == cam;
            const uint64_t m = __ballot(in);
            const int at = n + __popcll(m & ((1ull << lane) - 1));
            if (in && at < CALIB_VIEWS_PER_CAMERA_MAX) s_list[at] = v;
            n += __popcll(m);
        }
        if (lane == 0) s_cam.nused = n;
    }
    __syncthreads();
    CalibDevExec<CALIB_SOLVE_WAVES> x{s_lds[wv], tid, lane, wv};
    calib_camera(x, s_cam, s_list, j, cam);
}

hipError_t launch_calib(const CalibJob& j, hipStream_t s)
{
    hipError_t e = launch(k_calib_homography, dim3((unsigned)calib_homography_workgroups(j.n_views)), dim3(64 * CALIB_HOMOGRAPHY_WAVES), 0, s, j);
    if (e != hipSuccess) return e;
    return launch(k_calib_solve, dim3((unsigned)j.n_cameras), dim3(64 * CALIB_SOLVE_WAVES), 0, s, j);
}

} // namespace rmcv
