// model_plan.h -- the icon classifier's model table: the rule from a frame's raw model index to a table entry, the entry's
// device layout, how a host model is packed into it and what a table refuses -- decided before any GPU work.  Pure functions of plain
// values, without HIP types, so that a host compiler alone can check them (tests/test_model_plan.py); the rule is also what
// k_classify_models runs on the device.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/rmcv_abi.h"

#ifndef RMCV_PLAN_FN
#ifdef __HIPCC__
#define RMCV_PLAN_FN __host__ __device__ inline
#else
#define RMCV_PLAN_FN inline
#endif
#endif

namespace rmcv {

static constexpr int SVM_MAX_MODELS = RMCV_SVM_MAX_MODELS; // entries of a context's table: about 135 KB each, under 9 MB per context
static constexpr int MODEL_MAX_CLASSES = 8, MODEL_MAX_DF = 28, MODEL_NFEAT = RMCV_SVM_FEATURES;

// ---- the effective model of a frame, the one place it is computed -- by k_classify_models on the device, by rmcv_frame_model and the host
// setter on the host: a raw index, any int32 (a device-side producer may write it), -> an entry of the context's model table.
// Every value outside 0 .. n_models - 1 is model 0.
RMCV_PLAN_FN int32_t frame_model_eff(int32_t idx, int32_t n_models) { return ((uint32_t)idx < (uint32_t)n_models) ? idx : 0; }

// ---- one entry of the table as the device holds it: a fixed stride, 16-byte aligned, so that every weight row keeps its float4 loads
// (a row is 4800 bytes).  Decision functions and labels the model does not have are zero.
struct alignas(16) SvmModelEntry {
    float weights[MODEL_MAX_DF][MODEL_NFEAT]; // decision function d = (i, j), i < j, row-major, as rmcv_svm_load takes them
    double rho[MODEL_MAX_DF];
    int32_t labels[MODEL_MAX_CLASSES];
    int32_t n_class;
    int32_t pad_[3];
};
static_assert(sizeof(SvmModelEntry) == 134672 && sizeof(SvmModelEntry) % 16 == 0, "the table's stride");
static_assert(offsetof(SvmModelEntry, rho) == 134400 && offsetof(SvmModelEntry, labels) == 134624 && offsetof(SvmModelEntry, n_class) == 134656,
              "the entry's layout");

inline int model_n_df(int n_class) { return n_class * (n_class - 1) / 2; }

// a value that is neither an infinity nor a NaN (no <cmath>: the same text for every compiler and flag set)
inline bool model_finite(double v) { return v - v == 0.0; }

// What a table of n_models host models refuses: the message, or null.  buf: where a message that names an entry is written.
// Order: the count, then entry by entry: a null pointer, the class count, a non-finite weight, a non-finite rho.
inline const char* models_refusal(const rmcv_svm_model* models, int n_models, char (&buf)[200])
{
    if (n_models < 1 || n_models > SVM_MAX_MODELS) {
        snprintf(buf, sizeof(buf), "rmcv_svm_load_models: n_models %d is out of range (1 .. %d)", n_models, SVM_MAX_MODELS);
        return buf;
    }
    if (!models) return "rmcv_svm_load_models: a null pointer";
    for (int m = 0; m < n_models; m++) {
        const rmcv_svm_model& M = models[m];
        if (!M.weights || !M.rho || !M.labels) {
            snprintf(buf, sizeof(buf), "rmcv_svm_load_models: model %d: a null pointer", m);
            return buf;
        }
        if (M.n_class < 2 || M.n_class > MODEL_MAX_CLASSES) {
            snprintf(buf, sizeof(buf), "rmcv_svm_load_models: model %d: n_class %d is out of range (2 .. %d)", m, (int)M.n_class, MODEL_MAX_CLASSES);
            return buf;
        }
        const int n_df = model_n_df(M.n_class);
        for (size_t k = 0; k < (size_t)n_df * MODEL_NFEAT; k++)
            if (!model_finite(M.weights[k])) {
                snprintf(buf, sizeof(buf), "rmcv_svm_load_models: model %d: weight %d of decision function %d is not finite", m, (int)(k % MODEL_NFEAT), (int)(k / MODEL_NFEAT));
                return buf;
            }
        for (int d = 0; d < n_df; d++)
            if (!model_finite(M.rho[d])) {
                snprintf(buf, sizeof(buf), "rmcv_svm_load_models: model %d: rho %d is not finite", m, d);
                return buf;
            }
    }
    return nullptr;
}

// a host model models_refusal has passed (or rmcv_svm_load's arguments) -> its entry; everything the model does not have is zero
inline void model_pack(const rmcv_svm_model& M, SvmModelEntry* e)
{
    memset(e, 0, sizeof(*e));
    const int n_df = model_n_df(M.n_class);
    memcpy(e->weights, M.weights, (size_t)n_df * MODEL_NFEAT * sizeof(float));
    memcpy(e->rho, M.rho, (size_t)n_df * sizeof(double));
    memcpy(e->labels, M.labels, (size_t)M.n_class * sizeof(int32_t));
    e->n_class = M.n_class;
}

// what the host setter refuses of its indices: the first frame whose index is not an entry, or -1
inline int frame_models_outside(const int32_t* idx, int n_frames, int n_models)
{
    for (int f = 0; f < n_frames; f++)
        if (frame_model_eff(idx[f], n_models) != idx[f]) return f;
    return -1;
}
inline const char* frame_models_refusal(const int32_t* idx, int n_frames, int n_models, char (&buf)[200])
{
    const int f = frame_models_outside(idx, n_frames, n_models);
    if (f < 0) return nullptr;
    snprintf(buf, sizeof(buf), "rmcv_batch_set_frame_models: frame %d: model %d is outside the table (0 .. %d)", f, (int)idx[f], n_models - 1);
    return buf;
}

// the sticky model index table (rmcv_pipeline_set_frame_models) of a batch with RMCV_STAGE_IDENTITY: one index per frame, and every slot's
// context must hold a table of the same size -- the batch runs in whichever slot its ticket gives it
inline const char* pipeline_models_refusal(int n_frames, int idx_frames, bool tables_agree, char (&buf)[200])
{
    if (n_frames == idx_frames)
        return tables_agree ? nullptr : "n_models differs between the pipeline's contexts: load the same models into EVERY slot (rmcv_pipeline_context, rmcv_svm_load_models)";
    snprintf(buf, sizeof(buf), "the batch has %d frames, the pipeline's model index table %d (rmcv_pipeline_set_frame_models)", n_frames, idx_frames);
    return buf;
}

} // namespace rmcv
