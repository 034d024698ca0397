// k_classify_models.hip -- the icon classifier of a batch with per-frame models: frame f is classified with entry
// frame_model_eff(idx[f], n_models) of the context's model table (model_plan.h), the reference's svm_red / svm_blue
// (executable/main.cpp:21-22) for a mixed fleet's batch.
//
// One launch over the whole batch, one wavefront per (frame, armour): workgroup (f, q) holds the armours 4q .. 4q + 3 of frame f, a wave
// whose armour lies at or beyond min(n_armours[f], max_armours) leaves at once.  No count is read on the host and nothing is launched
// twice; a frame with 13 armours occupies four workgroups side by side where k_classify's one workgroup walks them in four passes.
// The frame, and with it the model index and the entry's address, is the workgroup's: one scalar load of idx[f], the entry's base in
// scalar registers, weight rows addressed from it.  The icon is icon_row's (device_classify.h), the decision and vote arithmetic is
// classify_frame's, restated: 21 (at most 28) lanes, each a sequential dot product in feature order in double, 4-bit vote counters --
// order dependent and pinned.  LDS is per wave only (the features and the sums); no wave waits for another.
#include "device_classify.h"
#include "model_plan.h"

namespace rmcv {

// BAYER: 0 BGR frames (win_eff nullable: the frames' window origins), 1 mosaics of `pattern` in the layout `lay`, 2 BGR frames read
// through their gamma tables `luts`.  model_eff[f] = the entry used (what rmcv_batch_get_frame_models reads), for every frame of the grid.
template <int BAYER>
__global__ __launch_bounds__(256) void k_classify_models(ClassifyArgs C, rmcv_armour* __restrict__ armours, const int32_t* __restrict__ n_armours,
                                                        int max_armours, const SvmModelEntry* __restrict__ table, const int32_t* __restrict__ idx,
                                                        int n_models, int32_t* __restrict__ model_eff, const rmcv_point* __restrict__ win_eff,
                                                        int pattern, int lay, const uint8_t* __restrict__ luts)
{
    __shared__ float s_feat[4][NFEAT];
    __shared__ double s_sum[4][32];
    const int f = blockIdx.x, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int a = blockIdx.y * 4 + wave;
    const int m = __builtin_amdgcn_readfirstlane(frame_model_eff(idx[f], n_models));
    if (a == 0 && lane == 0) model_eff[f] = m;
    const int n_f = n_armours[f], n = n_f < max_armours ? n_f : max_armours;
    if (a >= n) return;
    const SvmModelEntry* __restrict__ E = table + m;
    const int n_class = __builtin_amdgcn_readfirstlane(E->n_class);
    float* feat = s_feat[wave];
    double* sums = s_sum[wave];
    int64_t origin = 0;
    if constexpr (BAYER == 0) origin = frame_origin_offset(win_eff, f, C.stride);
    const uint8_t* frame = C.frames + (int64_t)f * C.frame_pitch + origin;
    int32_t* __restrict__ identity = C.identity;
    uint8_t* __restrict__ icons = C.icons;
    rmcv_armour* A = armours + (int64_t)f * max_armours + a;
    float ic[4][2];
    icon_row<BAYER>(frame, f, lane, A, C.w, C.h, C.stride, pattern, lay, luts, ic, [&](int o, const int (&res)[3]) __attribute__((always_inline)) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            feat[o * 3 + c] = (float)res[c]; // flatten_image: reshape(1,1), CV_32FC1
            if (icons) icons[((int64_t)f * max_armours + a) * NFEAT + o * 3 + c] = (uint8_t)res[c];
        }
    });
    __builtin_amdgcn_wave_barrier();
    // ---- main.cpp:181 svm->predict: one lane per decision function (classify_frame's arithmetic, term for term)
    const int n_df = n_class * (n_class - 1) / 2;
    if (lane < n_df) {
        const float* wv = E->weights[lane];
        double s = 0;
        for (int k = 0; k < NFEAT; k += 4) {
            const float4 wq = *reinterpret_cast<const float4*>(wv + k);
            s += wq.x * feat[k] + wq.y * feat[k + 1] + wq.z * feat[k + 2] + wq.w * feat[k + 3];
        }
        const float kval = (float)(s * 1.0 + 0.0);
        sums[lane] = -E->rho[lane] + 1.0 * kval;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        // votes of the (at most 8) classes as eight 4-bit counters of one word (a class meets at most 7 others)
        uint32_t votes = 0;
        int dfi = 0;
        for (int i = 0; i < n_class; i++)
            for (int j = i + 1; j < n_class; j++, dfi++) votes += 1u << (4 * (sums[dfi] > 0 ? i : j));
        int best = 0, bv_ = (int)(votes & 15u);
#pragma unroll
        for (int q = 1; q < 8; q++) {
            const int vq = (int)((votes >> (4 * q)) & 15u);
            if (q < n_class && vq > bv_) { best = q; bv_ = vq; }
        }
        identity[(int64_t)f * max_armours + a] = E->labels[best];
#pragma unroll
        for (int i = 0; i < 4; i++) { A->icon[i][0] = ic[i][0]; A->icon[i][1] = ic[i][1]; }
    }
}

hipError_t launch_classify_models(const Geom& g, const Bufs& b, const Limits& lim, hipStream_t s)
{
    ClassifyArgs C = classify_args(g, b); // (the single model's pointers are not read: every frame's come from its entry)
    C.weights = nullptr, C.rho = nullptr, C.labels = nullptr, C.n_class = 0;
    const dim3 grid(g.n_frames, lim.max_armours > 4 ? (lim.max_armours + 3) / 4 : 1), block(256);
    if (g.input_format != RMCV_INPUT_BGR)
        return launch(k_classify_models<1>, grid, block, 0, s, C, b.armours, b.n_armours, lim.max_armours, b.svm_table, b.model_idx, b.svm_models, b.model_eff,
                      nullptr, g.input_format, raw_layout(8 * g.sample_bytes, g.valid_bit, g.orient), nullptr);
    if (g.enhance)
        return launch(k_classify_models<2>, grid, block, 0, s, C, b.armours, b.n_armours, lim.max_armours, b.svm_table, b.model_idx, b.svm_models, b.model_eff,
                      nullptr, 0, 0, b.enh_lut);
    return launch(k_classify_models<0>, grid, block, 0, s, C, b.armours, b.n_armours, lim.max_armours, b.svm_table, b.model_idx, b.svm_models, b.model_eff,
                  g.win ? b.win_eff : nullptr, 0, 0, nullptr);
}

} // namespace rmcv
