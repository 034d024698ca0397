// rmcv_svm.hip -- the host side of the icon classifier's trainer: rmcv_svm_train / _gram / _predict on the device, and their
// sequential forms rmcv_svm_train_host / _gram_host / _predict_host (no context, no GPU).  What a call decides is svm_plan.h's, decided
// before any GPU work; the kernels are k_svm.hip's.  Training is no `submit`: its workspace is allocated per call and freed on every path
// (SvmScratch's destructor), and every wait polls against the context's deadline.
#include "rmcv_ctx.h"

using namespace rmcv;

namespace {

// device memory of one call
struct SvmScratch {
    std::vector<void*> blocks;
    hipEvent_t ev[8] = {}; // around the six phases of a training call (rmcv_svm_train_report::phase_ms)
    ~SvmScratch()
    {
        for (void* p : blocks) hipFree(p);
        for (hipEvent_t e : ev)
            if (e) hipEventDestroy(e);
    }
    hipError_t events()
    {
        hipError_t e = hipSuccess;
        for (int k = 0; k < 8 && e == hipSuccess; k++) e = hipEventCreate(&ev[k]);
        return e;
    }
    template <typename T>
    hipError_t get(T** p, size_t bytes)
    {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes ? bytes : 1);
        if (e == hipSuccess) blocks.push_back(q);
        *p = static_cast<T*>(q);
        return e;
    }
};

// an event of the phase timing behind what is enqueued (not a HIPCHK: a wait that runs out names the KERNEL enqueued last)
#define SVM_MARK(c, ws, k, s)                                                           \
    do {                                                                                \
        const hipError_t em__ = hipEventRecord((ws).ev[k], (s));                        \
        if (em__ != hipSuccess) return fail((c), RMCV_ERR_HIP, "hipEventRecord", em__); \
    } while (0)

int refuse_train(rmcv_ctx* c, rmcv_svm_train_report* report, const char* why)
{
    svm_report_reset(report, why);
    return fail(c, RMCV_ERR_BAD_ARG, why);
}

} // namespace

extern "C" {

void rmcv_svm_train_defaults(rmcv_svm_train_params* out)
{
    if (out) svm_default_params(out);
}

int rmcv_svm_gram_host(const uint8_t* samples, int n, int32_t* gram_out)
{
    if (!samples || !gram_out || n < 1 || n > RMCV_SVM_MAX_SAMPLES) return RMCV_ERR_BAD_ARG;
    svm_gram_seq(samples, n, gram_out);
    return RMCV_OK;
}

int rmcv_svm_predict_host(const float* weights, const double* rho, const int32_t* labels, int n_class, const uint8_t* samples, int n, int32_t* identity_out)
{
    if (!weights || !rho || !labels || n_class < 2 || n_class > 8 || n < 0 || (n && (!samples || !identity_out))) return RMCV_ERR_BAD_ARG;
    std::vector<float> feat(SVM_NFEAT);
    double sums[RMCV_SVM_MAX_DF];
    for (int r = 0; r < n; r++) identity_out[r] = labels[svm_predict_row(weights, rho, n_class, samples + (size_t)r * SVM_NFEAT, feat.data(), sums)];
    return RMCV_OK;
}

int rmcv_svm_train_host(const uint8_t* samples, const int32_t* responses, int n, const int32_t* perm, const rmcv_svm_train_params* params,
                        float* weights_out, double* rho_out, int32_t* labels_out, int32_t* n_class_out, rmcv_svm_train_report* report)
{
    svm_report_reset(report, nullptr);
    if (!samples || !responses || !weights_out || !rho_out || !labels_out || !n_class_out) return refuse_train(nullptr, report, "svm train: a null pointer");
    rmcv_svm_train_params p;
    if (params) p = *params;
    else svm_default_params(&p);
    if (const char* why = svm_train_seq(samples, responses, n, perm, p, weights_out, rho_out, labels_out, n_class_out, report)) return refuse_train(nullptr, report, why);
    return RMCV_OK;
}

int rmcv_svm_gram(rmcv_ctx* c, const uint8_t* samples, int n, int32_t* gram_out)
{
    if (!c || !samples || !gram_out || n < 1 || n > RMCV_SVM_MAX_SAMPLES) return RMCV_ERR_BAD_ARG;
    if (const int rc = ctx_ready(c)) return rc;
    SvmScratch ws;
    uint8_t* d_samples = nullptr;
    int32_t* d_gram = nullptr;
    hipError_t e = ws.get(&d_samples, (size_t)n * SVM_NFEAT);
    if (e == hipSuccess) e = ws.get(&d_gram, (size_t)n * n * sizeof(int32_t));
    if (e != hipSuccess) return fail(c, RMCV_ERR_NOMEM, "svm gram workspace", e);
    HIPCHK(c, hipMemcpy(d_samples, samples, (size_t)n * SVM_NFEAT, hipMemcpyHostToDevice), "H2D svm samples");
    HIPCHK(c, launch_svm_gram(d_samples, n, d_gram, c->stream), "k_svm_gram");
    WAITCHK(c, wait_stream(c, c->stream, "rmcv_svm_gram"));
    HIPCHK(c, hipMemcpy(gram_out, d_gram, (size_t)n * n * sizeof(int32_t), hipMemcpyDeviceToHost), "D2H svm gram");
    return RMCV_OK;
}

int rmcv_svm_predict(rmcv_ctx* c, const uint8_t* samples, int n, int32_t* identity_out)
{
    if (!c || n < 0 || (n && (!samples || !identity_out))) return RMCV_ERR_BAD_ARG;
    return svm_predict_rows(c, nullptr, samples, n, identity_out);
}

int rmcv_svm_predict_model(rmcv_ctx* c, int model, const uint8_t* samples, int n, int32_t* identity_out)
{
    if (!c || n < 0 || (n && (!samples || !identity_out))) return RMCV_ERR_BAD_ARG;
    if (!c->bufs.svm_w) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_svm_predict needs a model: rmcv_svm_load first");
    if (model < 0 || model >= c->bufs.svm_models) {
        char msg[160];
        snprintf(msg, sizeof(msg), "rmcv_svm_predict_model: model %d is outside the table (0 .. %d)", model, c->bufs.svm_models - 1);
        return fail(c, RMCV_ERR_BAD_ARG, msg);
    }
    return svm_predict_rows(c, nullptr, samples, n, identity_out, model);
}

int rmcv_svm_train(rmcv_ctx* c, const uint8_t* samples, const int32_t* responses, int n, const int32_t* perm, const rmcv_svm_train_params* params,
                   float* weights_out, double* rho_out, int32_t* labels_out, int32_t* n_class_out, rmcv_svm_train_report* report)
{
    svm_report_reset(report, nullptr);
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!samples || !responses || !weights_out || !rho_out || !labels_out || !n_class_out) return refuse_train(c, report, "svm train: a null pointer");
    return svm_train_rows(c, nullptr, samples, responses, n, perm, params, weights_out, rho_out, labels_out, n_class_out, report);
}

} // extern "C"

namespace rmcv {

int svm_predict_rows(rmcv_ctx* c, const uint8_t* d_rows, const uint8_t* samples, int n, int32_t* identity_out, int model)
{
    if (!c->bufs.svm_w) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_svm_predict needs a model: rmcv_svm_load first");
    if (n > (1 << 20)) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_svm_predict: more than 1048576 rows in one call");
    if (n == 0) return RMCV_OK;
    if (const int rc = ctx_ready(c)) return rc;
    SvmScratch ws;
    uint8_t* d_samples = const_cast<uint8_t*>(d_rows); // (only read)
    int32_t* d_out = nullptr;
    hipError_t e = d_rows ? hipSuccess : ws.get(&d_samples, (size_t)n * SVM_NFEAT);
    if (e == hipSuccess) e = ws.get(&d_out, (size_t)n * sizeof(int32_t));
    if (e != hipSuccess) return fail(c, RMCV_ERR_NOMEM, "svm predict workspace", e);
    if (!d_rows) HIPCHK(c, hipMemcpy(d_samples, samples, (size_t)n * SVM_NFEAT, hipMemcpyHostToDevice), "H2D svm samples");
    if (model >= 0) { // the entry's own rows of the table: the same kernel, the same arithmetic
        const SvmModelEntry* E = c->bufs.svm_table + model;
        HIPCHK(c, launch_svm_predict(d_samples, n, &E->weights[0][0], E->rho, c->model_classes[model], nullptr, 0, 1, E->labels, d_out, c->stream), "k_svm_predict");
    } else
        HIPCHK(c, launch_svm_predict(d_samples, n, c->bufs.svm_w, c->bufs.svm_rho, c->bufs.svm_classes, nullptr, 0, 1, c->bufs.svm_labels, d_out, c->stream), "k_svm_predict");
    WAITCHK(c, wait_stream(c, c->stream, "rmcv_svm_predict"));
    HIPCHK(c, hipMemcpy(identity_out, d_out, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost), "D2H svm identities");
    return RMCV_OK;
}

int svm_train_rows(rmcv_ctx* c, const uint8_t* d_rows, const uint8_t* samples, const int32_t* responses, int n, const int32_t* perm,
                   const rmcv_svm_train_params* params, float* weights_out, double* rho_out, int32_t* labels_out, int32_t* n_class_out,
                   rmcv_svm_train_report* report)
{
    rmcv_svm_train_params p;
    if (params) p = *params;
    else svm_default_params(&p);
    // ---- everything the call decides, before any GPU work
    SvmPlan pl;
    if (const char* why = svm_plan_build(pl, responses, n, perm, p)) return refuse_train(c, report, why);
    const SvmWorkspace sz = svm_workspace(pl);
    if (const int rc = ctx_ready(c)) return rc;
    hipStream_t s = c->stream;
    // ---- the workspace
    SvmScratch ws;
    uint8_t* d_samples = const_cast<uint8_t*>(d_rows); // (only read)
    int32_t *d_gram = nullptr, *d_cls = nullptr, *d_lists = nullptr, *d_fold_of = nullptr, *d_pred = nullptr;
    SvmProblem* d_problems = nullptr;
    double *d_alphas = nullptr, *d_rho = nullptr;
    float* d_weights = nullptr;
    SvmPairOut* d_outs = nullptr;
    hipError_t e = d_rows ? hipSuccess : ws.get(&d_samples, sz.samples);
    if (e == hipSuccess) e = ws.get(&d_gram, sz.gram);
    if (e == hipSuccess) e = ws.get(&d_cls, sz.cls);
    if (e == hipSuccess) e = ws.get(&d_lists, sz.lists);
    if (e == hipSuccess) e = ws.get(&d_problems, sz.problems);
    if (e == hipSuccess) e = ws.get(&d_alphas, sz.alphas);
    if (e == hipSuccess) e = ws.get(&d_weights, sz.weights);
    if (e == hipSuccess) e = ws.get(&d_rho, sz.rho);
    if (e == hipSuccess) e = ws.get(&d_outs, sz.outs);
    if (e == hipSuccess) e = ws.get(&d_fold_of, sz.fold_of);
    if (e == hipSuccess) e = ws.get(&d_pred, sz.pred);
    if (e == hipSuccess) e = ws.events();
    if (e != hipSuccess) return fail(c, RMCV_ERR_NOMEM, "svm train workspace", e);
    if (!d_rows) HIPCHK(c, hipMemcpy(d_samples, samples, sz.samples, hipMemcpyHostToDevice), "H2D svm samples");
    HIPCHK(c, hipMemcpy(d_cls, pl.cls.data(), sz.cls, hipMemcpyHostToDevice), "H2D svm classes");
    HIPCHK(c, hipMemcpy(d_lists, pl.lists.data(), sz.lists, hipMemcpyHostToDevice), "H2D svm lists");
    const SvmDevice dev{d_samples, d_gram, n, d_cls, d_lists, d_problems, d_alphas, d_weights, d_rho, d_outs};
    SVM_MARK(c, ws, 0, s);
    HIPCHK(c, launch_svm_gram(d_samples, n, d_gram, s), "k_svm_gram");
    SVM_MARK(c, ws, 1, s);
    // ---- the grid search: every (grid entry, fold, pair) problem at once, then every row under the models that did not see it
    int32_t cv_errors[RMCV_SVM_MAX_GRID];
    int best = 0;
    if (pl.k_fold) {
        HIPCHK(c, hipMemcpy(d_fold_of, pl.fold_of.data(), sz.fold_of, hipMemcpyHostToDevice), "H2D svm folds");
        HIPCHK(c, hipMemcpy(d_problems, pl.search.data(), pl.search.size() * sizeof(SvmProblem), hipMemcpyHostToDevice), "H2D svm problems");
        HIPCHK(c, launch_svm_solve(dev, (int)pl.search.size(), pl.eps, pl.max_iter, s, ws.ev[2]), "k_svm_smo");
        SVM_MARK(c, ws, 3, s);
        HIPCHK(c, launch_svm_predict(d_samples, n, d_weights, d_rho, pl.n_class, d_fold_of, pl.k_fold, pl.n_c, nullptr, d_pred, s), "k_svm_predict");
        SVM_MARK(c, ws, 4, s);
        WAITCHK(c, wait_stream(c, s, "rmcv_svm_train (grid search)"));
        std::vector<int32_t> pred((size_t)pl.n_c * n);
        HIPCHK(c, hipMemcpy(pred.data(), d_pred, sz.pred, hipMemcpyDeviceToHost), "D2H svm predictions");
        for (int g = 0; g < pl.n_c; g++) {
            cv_errors[g] = 0;
            for (int r = 0; r < n; r++) cv_errors[g] += pred[(size_t)g * n + r] != pl.cls[r];
        }
        best = svm_best_entry(cv_errors, pl.n_c);
    }
    // ---- the returned model: all rows at the chosen C
    svm_plan_set_final(pl, p.c_grid[best]);
    HIPCHK(c, hipMemcpy(d_problems, pl.fin.data(), pl.fin.size() * sizeof(SvmProblem), hipMemcpyHostToDevice), "H2D svm problems");
    SVM_MARK(c, ws, 7, s);
    HIPCHK(c, launch_svm_solve(dev, pl.n_df, pl.eps, pl.max_iter, s, ws.ev[5]), "k_svm_smo");
    SVM_MARK(c, ws, 6, s);
    WAITCHK(c, wait_stream(c, s, "rmcv_svm_train (final training)"));
    std::vector<double> alphas((size_t)pl.fin_alphas);
    std::vector<SvmPairOut> outs(pl.n_df);
    HIPCHK(c, hipMemcpy(weights_out, d_weights, (size_t)pl.n_df * SVM_NFEAT * sizeof(float), hipMemcpyDeviceToHost), "D2H svm weights");
    HIPCHK(c, hipMemcpy(rho_out, d_rho, (size_t)pl.n_df * sizeof(double), hipMemcpyDeviceToHost), "D2H svm rho");
    HIPCHK(c, hipMemcpy(alphas.data(), d_alphas, alphas.size() * sizeof(double), hipMemcpyDeviceToHost), "D2H svm alphas");
    HIPCHK(c, hipMemcpy(outs.data(), d_outs, outs.size() * sizeof(SvmPairOut), hipMemcpyDeviceToHost), "D2H svm reports");
    for (int i = 0; i < pl.n_class; i++) labels_out[i] = pl.labels[i];
    *n_class_out = pl.n_class;
    svm_report_final(pl, pl.n_c, pl.k_fold ? cv_errors : nullptr, best, outs.data(), alphas.data(), report);
    if (report) { // GPU time between the events of each phase; a call without a search leaves the search's three at 0
        const int from[6] = {0, 1, 2, 3, 7, 5}, to[6] = {1, 2, 3, 4, 5, 6};
        for (int k = 0; k < 6; k++) {
            float ms = 0.0f;
            if (!pl.k_fold && k >= 1 && k <= 3) continue;
            if (hipEventElapsedTime(&ms, ws.ev[from[k]], ws.ev[to[k]]) == hipSuccess) report->phase_ms[k] = ms;
        }
        (void)hipGetLastError();
    }
    return RMCV_OK;
}

} // namespace rmcv
