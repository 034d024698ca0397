// svm_plan.h -- what a training call decides before anything runs, as pure functions a host compiler checks
// (tests/test_svm_plan.py): the class table, the problem table (grid entry, fold, pair) -> sample list, the workspace sizes, the limits
// and every refusal; and the sequential form of the whole call (svm_train_seq: rmcv_svm_train_host, and what the device path equals).
// No HIP here: rmcv_svm.hip runs the same plan through k_svm.hip's kernels.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "../../include/rmcv_abi.h"
#include "device_svm.h"

namespace rmcv {

static constexpr int SVM_GRAM_TILE = 64; // rows and columns of k_svm_gram's output tile

// one pair problem: rows lists[list_off .. list_off + n) (ascending dataset order) of classes ci < cj at cost C
struct SvmProblem {
    int32_t list_off, n, ci, cj;
    int32_t c_idx, fold; // the grid entry and fold of a search problem; -1, -1: a problem of the returned model
    int64_t alpha_off;   // its alphas in the workspace
    double C;
};

struct SvmPlan {
    int n = 0, n_class = 0, n_df = 0, n_c = 1, k_fold = 0; // k_fold 0: no search
    double eps = 0;
    int max_iter = 0;
    std::vector<int32_t> labels;  // [n_class] the distinct responses, ascending
    std::vector<int32_t> cls;     // [n] row -> class index
    std::vector<int32_t> perm;    // [n]
    std::vector<int32_t> fold_of; // [n] row -> the fold that tests it (search only)
    std::vector<int32_t> lists;   // the sample lists: [fold][pair] of the search, then [pair] of the final training
    std::vector<SvmProblem> search; // [(c * k_fold + fold) * n_df + pair]
    std::vector<SvmProblem> fin;    // [pair]; C is set by svm_plan_set_final
    int64_t search_alphas = 0, fin_alphas = 0;
};

inline void svm_default_params(rmcv_svm_train_params* p)
{
    memset(p, 0, sizeof(*p));
    p->eps = 1e-3;
    p->max_iter = 1000;
    p->k_fold = 10;
    p->n_c = 6;
    double c = 0.1;
    for (int k = 0; k < 6; k++, c *= 5.0) p->c_grid[k] = c; // 0.1, 0.5, 2.5, 12.5, 62.5, 312.5 (each product rounded)
}

inline const char* svm_params_refusal(const rmcv_svm_train_params& p)
{
    if (!(p.eps >= 0.0) || !(p.eps - p.eps == 0.0)) return "svm train: eps must be finite and not negative";
    if (p.max_iter < 1) return "svm train: max_iter must be at least 1";
    if (p.k_fold > RMCV_SVM_MAX_FOLDS) return "svm train: more than RMCV_SVM_MAX_FOLDS folds";
    if (p.n_c < 1 || p.n_c > RMCV_SVM_MAX_GRID) return "svm train: n_c must be 1 .. RMCV_SVM_MAX_GRID";
    for (int k = 0; k < p.n_c; k++)
        if (!(p.c_grid[k] > 0.0) || !(p.c_grid[k] - p.c_grid[k] == 0.0)) return "svm train: every C must be finite and positive";
    return nullptr;
}

// first row of fold k of K over n rows
inline int svm_fold_begin(int k, int K, int n) { return (int)((int64_t)k * n / K); }

// builds the whole plan or says why not (then `pl` is unspecified); nothing here touches a device
inline const char* svm_plan_build(SvmPlan& pl, const int32_t* responses, int n, const int32_t* perm, const rmcv_svm_train_params& p)
{
    if (const char* why = svm_params_refusal(p)) return why;
    if (n < 2) return "svm train: fewer than 2 rows";
    if (n > RMCV_SVM_MAX_SAMPLES) return "svm train: more rows than RMCV_SVM_MAX_SAMPLES";
    pl = SvmPlan();
    pl.n = n;
    pl.eps = p.eps;
    pl.max_iter = p.max_iter;
    pl.labels.assign(responses, responses + n);
    std::sort(pl.labels.begin(), pl.labels.end());
    pl.labels.erase(std::unique(pl.labels.begin(), pl.labels.end()), pl.labels.end());
    if (pl.labels.size() < 2) return "svm train: fewer than 2 classes";
    if (pl.labels.size() > 8) return "svm train: more than 8 classes";
    pl.n_class = (int)pl.labels.size();
    pl.n_df = pl.n_class * (pl.n_class - 1) / 2;
    pl.cls.resize(n);
    std::vector<int> count(pl.n_class, 0);
    for (int r = 0; r < n; r++) {
        pl.cls[r] = (int32_t)(std::lower_bound(pl.labels.begin(), pl.labels.end(), responses[r]) - pl.labels.begin());
        count[pl.cls[r]]++;
    }
    pl.perm.resize(n);
    {
        std::vector<char> seen(n, 0);
        for (int r = 0; r < n; r++) {
            const int32_t q = perm ? perm[r] : r;
            if (q < 0 || q >= n || seen[q]) return "svm train: perm is not a permutation of the rows";
            seen[q] = 1;
            pl.perm[r] = q;
        }
    }
    for (int i = 0; i < pl.n_class; i++)
        for (int j = i + 1; j < pl.n_class; j++)
            if (count[i] + count[j] > RMCV_SVM_MAX_PAIR_SAMPLES) return "svm train: two classes have more rows together than RMCV_SVM_MAX_PAIR_SAMPLES";
    const bool search = p.k_fold > 1 && p.n_c > 1;
    pl.k_fold = search ? p.k_fold : 0;
    pl.n_c = search ? p.n_c : 1;
    std::vector<int32_t> fold_list_off, fold_list_n; // [fold][pair]
    if (search) {
        pl.fold_of.assign(n, 0);
        for (int k = 0; k < pl.k_fold; k++) {
            std::vector<int> left(count);
            for (int q = svm_fold_begin(k, pl.k_fold, n); q < svm_fold_begin(k + 1, pl.k_fold, n); q++) {
                pl.fold_of[pl.perm[q]] = k;
                left[pl.cls[pl.perm[q]]]--;
            }
            for (int i = 0; i < pl.n_class; i++)
                if (left[i] <= 0) return "svm train: the training part of a fold lacks a class";
        }
        for (int k = 0; k < pl.k_fold; k++)
            for (int i = 0; i < pl.n_class; i++)
                for (int j = i + 1; j < pl.n_class; j++) {
                    fold_list_off.push_back((int32_t)pl.lists.size());
                    for (int r = 0; r < n; r++)
                        if ((pl.cls[r] == i || pl.cls[r] == j) && pl.fold_of[r] != k) pl.lists.push_back(r);
                    fold_list_n.push_back((int32_t)pl.lists.size() - fold_list_off.back());
                }
        for (int c = 0; c < pl.n_c; c++)
            for (int k = 0; k < pl.k_fold; k++) {
                int d = 0;
                for (int i = 0; i < pl.n_class; i++)
                    for (int j = i + 1; j < pl.n_class; j++, d++) {
                        SvmProblem q{fold_list_off[k * pl.n_df + d], fold_list_n[k * pl.n_df + d], i, j, c, k, pl.search_alphas, p.c_grid[c]};
                        pl.search_alphas += q.n;
                        pl.search.push_back(q);
                    }
            }
    }
    for (int i = 0; i < pl.n_class; i++)
        for (int j = i + 1; j < pl.n_class; j++) {
            SvmProblem q{(int32_t)pl.lists.size(), 0, i, j, -1, -1, pl.fin_alphas, p.c_grid[0]};
            for (int r = 0; r < n; r++)
                if (pl.cls[r] == i || pl.cls[r] == j) pl.lists.push_back(r);
            q.n = (int32_t)pl.lists.size() - q.list_off;
            pl.fin_alphas += q.n;
            pl.fin.push_back(q);
        }
    return nullptr;
}

inline void svm_plan_set_final(SvmPlan& pl, double C)
{
    for (auto& q : pl.fin) q.C = C;
}

// the grid entry a search returns: the lowest error, the earlier entry on a tie
inline int svm_best_entry(const int32_t* cv_errors, int n_c)
{
    int best = 0;
    for (int c = 1; c < n_c; c++)
        if (cv_errors[c] < cv_errors[best]) best = c;
    return best;
}

// device workspace of a call, bytes per part (rmcv_svm.hip allocates exactly these)
struct SvmWorkspace {
    size_t samples, gram, cls, lists, problems, alphas, weights, rho, outs, fold_of, pred;
    size_t total() const { return samples + gram + cls + lists + problems + alphas + weights + rho + outs + fold_of + pred; }
};
inline SvmWorkspace svm_workspace(const SvmPlan& pl)
{
    const size_t n = (size_t)pl.n, probs = std::max(pl.search.size(), pl.fin.size());
    SvmWorkspace w;
    w.samples = n * SVM_NFEAT;
    w.gram = n * n * sizeof(int32_t);
    w.cls = n * sizeof(int32_t);
    w.lists = pl.lists.size() * sizeof(int32_t);
    w.problems = probs * sizeof(SvmProblem);
    w.alphas = (size_t)std::max(pl.search_alphas, pl.fin_alphas) * sizeof(double);
    w.weights = probs * SVM_NFEAT * sizeof(float);
    w.rho = probs * sizeof(double);
    w.outs = probs * sizeof(SvmPairOut);
    w.fold_of = n * sizeof(int32_t);
    w.pred = (size_t)pl.n_c * n * sizeof(int32_t);
    return w;
}

// the parts of the workspace as the kernels take them (device addresses)
struct SvmDevice {
    const uint8_t* samples;
    int32_t* gram;
    int n;
    const int32_t *cls, *lists;
    const SvmProblem* problems;
    double* alphas;
    float* weights;
    double* rho;
    SvmPairOut* outs;
};

// the report of a call that has not run yet
inline void svm_report_reset(rmcv_svm_train_report* r, const char* why)
{
    if (!r) return;
    double* keep = r->alpha_out;
    memset(r, 0, sizeof(*r));
    r->alpha_out = keep;
    for (int c = 0; c < RMCV_SVM_MAX_GRID; c++) r->cv_errors[c] = -1;
    r->best_index = -1;
    if (why) snprintf(r->message, sizeof(r->message), "%s", why);
}

// what a finished call hands out besides the model: the final problems' reports and alphas by dataset row
inline void svm_report_final(const SvmPlan& pl, int n_c, const int32_t* cv_errors, int best, const SvmPairOut* outs, const double* alphas,
                             rmcv_svm_train_report* r)
{
    if (!r) return;
    r->best_index = best;
    r->best_c = pl.fin[0].C;
    r->n_df = pl.n_df;
    for (int c = 0; c < n_c && cv_errors; c++) r->cv_errors[c] = cv_errors[c];
    for (int d = 0; d < pl.n_df; d++) {
        r->iterations[d] = outs[d].iterations;
        r->converged[d] = outs[d].converged;
        r->objective[d] = outs[d].objective;
    }
    if (r->alpha_out) {
        for (size_t k = 0; k < (size_t)pl.n_df * pl.n; k++) r->alpha_out[k] = 0.0;
        for (int d = 0; d < pl.n_df; d++)
            for (int t = 0; t < pl.fin[d].n; t++) r->alpha_out[(size_t)d * pl.n + pl.lists[pl.fin[d].list_off + t]] = alphas[pl.fin[d].alpha_off + t];
    }
}

// ---- the sequential form of a whole call -------------------------------------------------------------------------------------------
inline void svm_gram_seq(const uint8_t* samples, int n, int32_t* G)
{
    for (int a = 0; a < n; a++)
        for (int b = a; b < n; b++) G[(size_t)a * n + b] = G[(size_t)b * n + a] = svm_gram_entry(samples + (size_t)a * SVM_NFEAT, samples + (size_t)b * SVM_NFEAT);
}

// problems[0 .. count): alphas at their alpha_off, the models' weights [count][1200] and rho [count], the reports
inline double svm_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ms[0], ms[1] (nullable): wall time of the solver and of the weights, added up
inline void svm_solve_all_seq(const SvmPlan& pl, const SvmProblem* problems, size_t count, const uint8_t* samples, const int32_t* G, double* alphas,
                              float* weights, double* rho, SvmPairOut* outs, double* ms = nullptr)
{
    std::vector<int8_t> y(RMCV_SVM_MAX_PAIR_SAMPLES);
    std::vector<double> g(RMCV_SVM_MAX_PAIR_SAMPLES);
    for (size_t q = 0; q < count; q++) {
        const SvmProblem& P = problems[q];
        const int32_t* idx = pl.lists.data() + P.list_off;
        for (int t = 0; t < P.n; t++) y[t] = pl.cls[idx[t]] == P.ci ? 1 : -1;
        const double t0 = svm_now_ms();
        svm_solve_seq(G, pl.n, idx, y.data(), P.n, P.C, pl.eps, pl.max_iter, alphas + P.alpha_off, g.data(), &outs[q]);
        rho[q] = outs[q].rho;
        const double t1 = svm_now_ms();
        for (int k = 0; k < SVM_NFEAT; k++) weights[q * SVM_NFEAT + k] = svm_weight(samples, idx, y.data(), alphas + P.alpha_off, P.n, k);
        if (ms) { ms[0] += t1 - t0; ms[1] += svm_now_ms() - t1; }
    }
}

// rmcv_svm_train_host behind its argument checks; the outputs as the ABI describes them
inline const char* svm_train_seq(const uint8_t* samples, const int32_t* responses, int n, const int32_t* perm, const rmcv_svm_train_params& p,
                                 float* weights_out, double* rho_out, int32_t* labels_out, int32_t* n_class_out, rmcv_svm_train_report* report)
{
    SvmPlan pl;
    if (const char* why = svm_plan_build(pl, responses, n, perm, p)) return why;
    std::vector<int32_t> G((size_t)n * n);
    double ms[6] = {0, 0, 0, 0, 0, 0}; // rmcv_svm_train_report::phase_ms, wall time here
    const double t_gram = svm_now_ms();
    svm_gram_seq(samples, n, G.data());
    ms[0] = svm_now_ms() - t_gram;
    int32_t cv_errors[RMCV_SVM_MAX_GRID];
    int best = 0;
    if (pl.k_fold) {
        const size_t count = pl.search.size();
        std::vector<double> alphas((size_t)pl.search_alphas), rho(count);
        std::vector<float> weights(count * SVM_NFEAT), feat(SVM_NFEAT);
        std::vector<SvmPairOut> outs(count);
        svm_solve_all_seq(pl, pl.search.data(), count, samples, G.data(), alphas.data(), weights.data(), rho.data(), outs.data(), ms + 1);
        double sums[RMCV_SVM_MAX_DF];
        const double t_pred = svm_now_ms();
        for (int c = 0; c < pl.n_c; c++) {
            cv_errors[c] = 0;
            for (int r = 0; r < n; r++) {
                const size_t model = ((size_t)c * pl.k_fold + pl.fold_of[r]) * pl.n_df;
                cv_errors[c] += svm_predict_row(weights.data() + model * SVM_NFEAT, rho.data() + model, pl.n_class, samples + (size_t)r * SVM_NFEAT, feat.data(), sums) != pl.cls[r];
            }
        }
        best = svm_best_entry(cv_errors, pl.n_c);
        ms[3] = svm_now_ms() - t_pred;
    }
    svm_plan_set_final(pl, p.c_grid[best]);
    std::vector<double> alphas((size_t)pl.fin_alphas);
    std::vector<SvmPairOut> outs(pl.n_df);
    svm_solve_all_seq(pl, pl.fin.data(), pl.fin.size(), samples, G.data(), alphas.data(), weights_out, rho_out, outs.data(), ms + 4);
    for (int i = 0; i < pl.n_class; i++) labels_out[i] = pl.labels[i];
    *n_class_out = pl.n_class;
    svm_report_reset(report, nullptr);
    svm_report_final(pl, pl.n_c, pl.k_fold ? cv_errors : nullptr, best, outs.data(), alphas.data(), report);
    for (int k = 0; k < 6 && report; k++) report->phase_ms[k] = ms[k];
    return nullptr;
}

} // namespace rmcv
