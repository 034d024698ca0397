// k_svm.hip -- the kernels of the icon classifier's trainer (the rule: device_svm.h, the plan: svm_plan.h).
//   k_svm_gram     u8 [N][1200] -> int32 [N][N]: 64 x 64 output tiles, 80-byte slices of the rows in LDS, v_dot4_u32_u8
//                  (__builtin_amdgcn_udot4) on four bytes of a row pair at a time.  Exact integers: any order gives the same matrix.
//   k_svm_smo      one workgroup per pair problem: g, alpha, y and the row list live in LDS; selection = per-thread scan in ascending t,
//                  wave reduction, cross-wave reduction on the key (value, index); two Gram rows gathered per iteration; the loop is
//                  bounded by max_iter and no workgroup waits for another.
//   k_svm_weights  lane = feature, sequential over the pair's rows (svm_weight)
//   k_svm_predict  one wavefront per row, one lane per decision function (svm_decide: the arithmetic of device_classify.h:259-285)
#include "rmcv_internal.h"
#include "svm_plan.h"

namespace rmcv {

static constexpr int GRAM_KB = 80;                // bytes of a row per LDS slice: 1200 = 15 * 80
static constexpr int GRAM_KW = GRAM_KB / 4;       // ... as dwords
static constexpr int GRAM_LD = GRAM_KW + 1;       // LDS row stride in dwords: odd, so 16 rows 1 apart fall on 16 banks
static_assert(SVM_NFEAT % GRAM_KB == 0 && SVM_GRAM_TILE == 64, "tile shape");

// thread (tx, ty) of 16 x 16 owns outputs (ty + 16 q, tx + 16 p), q, p = 0 .. 3, of the tile: the 16 lanes of a row of threads read 16
// LDS rows one apart (no bank conflict) and store 16 consecutive ints
__global__ __launch_bounds__(256) void k_svm_gram(const uint8_t* __restrict__ samples, int n, int32_t* __restrict__ gram)
{
    __shared__ uint32_t s_a[SVM_GRAM_TILE * GRAM_LD], s_b[SVM_GRAM_TILE * GRAM_LD];
    const uint32_t* __restrict__ x = reinterpret_cast<const uint32_t*>(samples); // rows are 300 dwords apart
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int row0 = blockIdx.y * SVM_GRAM_TILE, col0 = blockIdx.x * SVM_GRAM_TILE;
    uint32_t acc[4][4] = {};
    for (int kt = 0; kt < SVM_NFEAT / GRAM_KB; kt++) {
        for (int e = tid; e < SVM_GRAM_TILE * GRAM_KW; e += 256) {
            const int r = e / GRAM_KW, c = e - r * GRAM_KW;
            const int ra = row0 + r, rb = col0 + r;
            s_a[r * GRAM_LD + c] = ra < n ? x[(int64_t)ra * (SVM_NFEAT / 4) + kt * GRAM_KW + c] : 0u;
            s_b[r * GRAM_LD + c] = rb < n ? x[(int64_t)rb * (SVM_NFEAT / 4) + kt * GRAM_KW + c] : 0u;
        }
        __syncthreads();
#pragma unroll 4
        for (int c = 0; c < GRAM_KW; c++) {
            uint32_t a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; q++) { a[q] = s_a[(ty + 16 * q) * GRAM_LD + c]; b[q] = s_b[(tx + 16 * q) * GRAM_LD + c]; }
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int p = 0; p < 4; p++) acc[q][p] = __builtin_amdgcn_udot4(a[q], b[p], acc[q][p], false);
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int r = row0 + ty + 16 * q, c = col0 + tx + 16 * p;
            if (r < n && c < n) gram[(int64_t)r * n + c] = (int32_t)acc[q][p];
        }
}

// ---- one pair problem per workgroup ----
__global__ __launch_bounds__(256) void k_svm_smo(const int32_t* __restrict__ gram, int n_rows, const int32_t* __restrict__ cls, const int32_t* __restrict__ lists,
                                                const SvmProblem* __restrict__ problems, double eps, int max_iter, double* __restrict__ alphas,
                                                double* __restrict__ rho, SvmPairOut* __restrict__ outs)
{
    __shared__ double s_g[RMCV_SVM_MAX_PAIR_SAMPLES], s_a[RMCV_SVM_MAX_PAIR_SAMPLES];
    __shared__ int32_t s_idx[RMCV_SVM_MAX_PAIR_SAMPLES];
    __shared__ int8_t s_y[RMCV_SVM_MAX_PAIR_SAMPLES];
    __shared__ double s_m[2][4], s_M[2][4]; // the waves' partial selections, two sets: iteration k + 1 writes the other one while k's is still read
    __shared__ int32_t s_i[2][4], s_j[2][4];
    const SvmProblem P = problems[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = P.n;
    if (n > RMCV_SVM_MAX_PAIR_SAMPLES) return; // (the plan refuses such a pair: never reached)
    const double C = P.C;
    for (int t = tid; t < n; t += 256) {
        const int32_t r = lists[P.list_off + t];
        s_idx[t] = r;
        s_y[t] = cls[r] == P.ci ? 1 : -1;
        s_a[t] = 0.0;
        s_g[t] = -1.0;
    }
    __syncthreads();
    int it = 0, conv = 0;
    for (;;) {
        const int par = it & 1;
        SvmSel s;
        svm_sel_init(&s);
        for (int t = tid; t < n; t += 256) svm_sel_offer(&s, t, s_y[t], s_a[t], s_g[t], C);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double om = __shfl_xor(s.m, off), oM = __shfl_xor(s.M, off);
            const int oi = __shfl_xor(s.i, off), oj = __shfl_xor(s.j, off);
            svm_sel_merge(&s, om, oi, oM, oj);
        }
        if (lane == 0) { s_m[par][wave] = s.m; s_M[par][wave] = s.M; s_i[par][wave] = s.i; s_j[par][wave] = s.j; }
        __syncthreads();
        svm_sel_init(&s);
#pragma unroll
        for (int w = 0; w < 4; w++) svm_sel_merge(&s, s_m[par][w], s_i[par][w], s_M[par][w], s_j[par][w]);
        if (svm_sel_done(&s, eps)) { conv = 1; break; } // (the same values in every thread: a uniform branch)
        if (it >= max_iter) break;
        const int yi = s_y[s.i], yj = s_y[s.j];
        const int32_t ri = s_idx[s.i], rj = s_idx[s.j];
        const int32_t* __restrict__ gi = gram + (int64_t)ri * n_rows;
        const int32_t* __restrict__ gj = gram + (int64_t)rj * n_rows;
        const SvmStep st = svm_step(yi, yj, s_a[s.i], s_a[s.j], s.m, s.M, svm_eta_int(gi[ri], gj[rj], gi[rj]), C);
        __syncthreads(); // every thread has read alpha_i and alpha_j
        for (int t = tid; t < n; t += 256) {
            const int32_t r = s_idx[t];
            const int yt = s_y[t];
            s_g[t] = svm_grad(s_g[t], svm_q(yt, yi, gi[r]), st.dai, svm_q(yt, yj, gj[r]), st.daj);
        }
        // the thread that scans t writes alpha_t: the next scan reads its own stores
        if ((s.i & 255) == tid) s_a[s.i] = st.ai;
        if ((s.j & 255) == tid) s_a[s.j] = st.aj;
        it++;
    }
    __syncthreads();
    for (int t = tid; t < n; t += 256) alphas[P.alpha_off + t] = s_a[t];
    if (tid == 0) {
        SvmPairOut out;
        svm_finish(s_y, s_a, s_g, n, C, &out);
        out.iterations = it;
        out.converged = conv;
        outs[blockIdx.x] = out;
        rho[blockIdx.x] = out.rho;
    }
}

// weights[problem][k] of the problem's alphas; grid (problems, ceil(1200 / 256))
__global__ __launch_bounds__(256) void k_svm_weights(const uint8_t* __restrict__ samples, const int32_t* __restrict__ cls, const int32_t* __restrict__ lists,
                                                    const SvmProblem* __restrict__ problems, const double* __restrict__ alphas, float* __restrict__ weights)
{
    __shared__ int32_t s_idx[RMCV_SVM_MAX_PAIR_SAMPLES];
    __shared__ int8_t s_y[RMCV_SVM_MAX_PAIR_SAMPLES];
    const SvmProblem P = problems[blockIdx.x];
    if (P.n > RMCV_SVM_MAX_PAIR_SAMPLES) return;
    for (int t = threadIdx.x; t < P.n; t += 256) {
        const int32_t r = lists[P.list_off + t];
        s_idx[t] = r;
        s_y[t] = cls[r] == P.ci ? 1 : -1;
    }
    __syncthreads();
    const int k = blockIdx.y * 256 + threadIdx.x;
    if (k < SVM_NFEAT) weights[(int64_t)blockIdx.x * SVM_NFEAT + k] = svm_weight(samples, s_idx, s_y, alphas + P.alpha_off, P.n, k);
}

// out[blockIdx.y * n + r] of row r under model (blockIdx.y * k_fold + fold_of[r]) (fold_of null: model 0): the class index, or labels[it]
__global__ __launch_bounds__(256) void k_svm_predict(const uint8_t* __restrict__ samples, int n, const float* __restrict__ weights, const double* __restrict__ rho,
                                                    int n_class, const int32_t* __restrict__ fold_of, int k_fold, const int32_t* __restrict__ labels,
                                                    int32_t* __restrict__ out)
{
    __shared__ float s_feat[4][SVM_NFEAT];
    __shared__ double s_sum[4][32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_df = n_class * (n_class - 1) / 2;
    for (int r = blockIdx.x * 4 + wave; r < n; r += gridDim.x * 4) {
        const int64_t model = fold_of ? ((int64_t)blockIdx.y * k_fold + fold_of[r]) * n_df : 0;
        for (int k = lane; k < SVM_NFEAT; k += 64) s_feat[wave][k] = (float)samples[(int64_t)r * SVM_NFEAT + k];
        __builtin_amdgcn_wave_barrier();
        if (lane < n_df) s_sum[wave][lane] = svm_decide(weights + (model + lane) * SVM_NFEAT, s_feat[wave], rho[model + lane]);
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            const int best = svm_vote(s_sum[wave], n_class);
            out[(int64_t)blockIdx.y * n + r] = labels ? labels[best] : best;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

hipError_t launch_svm_gram(const uint8_t* d_samples, int n, int32_t* d_gram, hipStream_t s)
{
    const int tiles = (n + SVM_GRAM_TILE - 1) / SVM_GRAM_TILE;
    return launch(k_svm_gram, dim3(tiles, tiles), dim3(256), 0, s, d_samples, n, d_gram);
}

hipError_t launch_svm_solve(const SvmDevice& d, int n_problems, double eps, int max_iter, hipStream_t s, hipEvent_t between)
{
    hipError_t e = launch(k_svm_smo, dim3(n_problems), dim3(256), 0, s, d.gram, d.n, d.cls, d.lists, d.problems, eps, max_iter, d.alphas, d.rho, d.outs);
    if (e == hipSuccess && between) e = hipEventRecord(between, s);
    if (e != hipSuccess) return e;
    return launch(k_svm_weights, dim3(n_problems, (SVM_NFEAT + 255) / 256), dim3(256), 0, s, d.samples, d.cls, d.lists, d.problems, d.alphas, d.weights);
}

hipError_t launch_svm_predict(const uint8_t* d_samples, int n, const float* d_weights, const double* d_rho, int n_class, const int32_t* d_fold_of, int k_fold,
                              int n_models, const int32_t* d_labels, int32_t* d_out, hipStream_t s)
{
    const int blocks = std::min((n + 3) / 4, 1024);
    return launch(k_svm_predict, dim3(blocks, n_models), dim3(256), 0, s, d_samples, n, d_weights, d_rho, n_class, d_fold_of, k_fold, d_labels, d_out);
}

} // namespace rmcv
