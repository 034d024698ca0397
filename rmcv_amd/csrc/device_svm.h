/*
 * device_svm.h -- the rule of the icon classifier's trainer, host and device from the same source: a linear one-vs-one
 * C-SVC as cv::ml::SVM trains it (executable/svm/optimizer.cpp:9-19), on the exact integer Gram matrix of the u8 rows.
 *   Gram        G[a][b] = sum_k x_a[k] * x_b[k], int32 (<= 1200 * 255^2 = 78 030 000), exact and order independent
 *   pair (i<j)  the rows of classes i and j in ascending dataset order, y = +1 for class i, -1 for class j, Q_tu = y_t y_u (double)G
 *   SMO         first-order "maximal violating pair" steps from alpha = 0, g = -1 (the form cv::ml::SVM's solver descends from)
 *   outputs     rho, w (f32), iterations, converged flag, dual objective
 *   predict     the arithmetic of device_classify.h:259-285, restated (tests prove the two equal)
 * Every floating-point operation below is one rounded IEEE operation in the order written: compile with -ffp-contract=off, no fast-math.
 *
 * Execution model.  The scalar pieces (svm_sel_*, svm_step, svm_q, svm_finish, svm_weight, svm_decide, svm_vote) are what BOTH forms run:
 * the sequential form (svm_solve_seq, below) loops over them; k_svm.hip's workgroup runs the selection as a reduction on the key
 * (value, index) and the gradient update one sample per thread.  Selection is a comparison of exact keys and the update is element-wise,
 * so the two forms agree bit for bit.  Arrays are indexed by loop counters over memory (LDS on the device), never registers.
 */
#ifndef RMCV_DEVICE_SVM_H
#define RMCV_DEVICE_SVM_H

#include <stdint.h>

#if defined(__HIPCC__)
#define SVM_FN __host__ __device__ static inline
#else
#define SVM_FN static inline
#endif

#define SVM_NFEAT 1200       /* RMCV_SVM_FEATURES */
#define SVM_ETA_FLOOR 1e-12  /* what a curvature that is not positive is replaced by */

/* ---- Gram ---- */
SVM_FN int32_t svm_gram_entry(const uint8_t* a, const uint8_t* b)
{
    int32_t s = 0;
    for (int k = 0; k < SVM_NFEAT; k++) s += (int32_t)a[k] * (int32_t)b[k];
    return s;
}

/* ---- selection ----
 * up  = (y = +1, alpha < C) u (y = -1, alpha > 0)      i = argmax over up  of v_t = -y_t g_t
 * low = (y = +1, alpha > 0) u (y = -1, alpha < C)      j = argmin over low of v_t
 * the lowest t wins a tie.  i (j) = -1: the set is empty. */
typedef struct { double m, M; int32_t i, j; } SvmSel;
SVM_FN int svm_in_up(int y, double a, double C) { return y > 0 ? a < C : a > 0.0; }
SVM_FN int svm_in_low(int y, double a, double C) { return y > 0 ? a > 0.0 : a < C; }
SVM_FN double svm_viol(int y, double g) { return y > 0 ? -g : g; } /* -y g, exact */
SVM_FN void svm_sel_init(SvmSel* s) { s->m = s->M = 0.0; s->i = s->j = -1; }
/* sample t, offered in ASCENDING t: only a strictly better value replaces the holder */
SVM_FN void svm_sel_offer(SvmSel* s, int t, int y, double a, double g, double C)
{
    const double v = svm_viol(y, g);
    if (svm_in_up(y, a, C) && (s->i < 0 || v > s->m)) { s->m = v; s->i = t; }
    if (svm_in_low(y, a, C) && (s->j < 0 || v < s->M)) { s->M = v; s->j = t; }
}
/* two partial selections in any order: the better value, the lower index between equal values */
SVM_FN void svm_sel_merge(SvmSel* s, double om, int oi, double oM, int oj)
{
    if (oi >= 0 && (s->i < 0 || om > s->m || (om == s->m && oi < s->i))) { s->m = om; s->i = oi; }
    if (oj >= 0 && (s->j < 0 || oM < s->M || (oM == s->M && oj < s->j))) { s->M = oM; s->j = oj; }
}
/* the solver stops (converged) on an empty set or a maximal violation below eps */
SVM_FN int svm_sel_done(const SvmSel* s, double eps) { return s->i < 0 || s->j < 0 || s->m - s->M < eps; }

/* ---- one step on the selected samples i (from up) and j (from low) ----
 * eta = K_ii + K_jj - 2 K_ij in integers, converted once; lambda = (m - M) / eta is the unclipped Newton step along
 * alpha_i += y_i lambda, alpha_j -= y_j lambda; it is cut to the room of i, then to the room of j; the sample whose room cut it last
 * lands on its bound exactly; both are kept inside [0, C]; the deltas are the differences of the stored values. */
typedef struct { double ai, aj, dai, daj; } SvmStep;
SVM_FN int64_t svm_eta_int(int32_t kii, int32_t kjj, int32_t kij) { return (int64_t)kii + (int64_t)kjj - 2 * (int64_t)kij; }
SVM_FN SvmStep svm_step(int yi, int yj, double ai, double aj, double m, double M, int64_t eta_int, double C)
{
    double eta = (double)eta_int;
    if (!(eta > 0.0)) eta = SVM_ETA_FLOOR;
    double lam = (m - M) / eta;
    const double room_i = yi > 0 ? C - ai : ai;
    const double room_j = yj > 0 ? aj : C - aj;
    int cut = 0;
    if (room_i < lam) { lam = room_i; cut = 1; }
    if (room_j < lam) { lam = room_j; cut = 2; }
    double ni = yi > 0 ? ai + lam : ai - lam;
    double nj = yj > 0 ? aj - lam : aj + lam;
    if (cut == 1) ni = yi > 0 ? C : 0.0;
    if (cut == 2) nj = yj > 0 ? 0.0 : C;
    if (ni > C) ni = C;
    if (ni < 0.0) ni = 0.0;
    if (nj > C) nj = C;
    if (nj < 0.0) nj = 0.0;
    SvmStep r;
    r.ai = ni;
    r.aj = nj;
    r.dai = ni - ai;
    r.daj = nj - aj;
    return r;
}
/* Q_tu = y_t y_u (double)G_tu: exact */
SVM_FN double svm_q(int yt, int yu, int32_t k) { return yt == yu ? (double)k : -(double)k; }
/* g_t after the step: two products and two sums, each rounded */
SVM_FN double svm_grad(double g, double qti, double dai, double qtj, double daj) { return (g + qti * dai) + qtj * daj; }

/* ---- what one pair problem reports besides its alphas ----
 * rho: the mean of y_t g_t over the free alphas (0 < alpha < C), summed in ascending t; without one, the midpoint of
 *      ub = min y_t g_t over (y = +1, alpha = 0) u (y = -1, alpha = C) and lb = max y_t g_t over the other bounded samples
 * objective: (sum_t alpha_t (g_t - 1)) / 2 in ascending t  (= 1/2 a'Qa - e'a while g = Qa - e) */
typedef struct { double rho, objective; int32_t iterations, converged; } SvmPairOut;
SVM_FN void svm_finish(const int8_t* y, const double* alpha, const double* g, int n, double C, SvmPairOut* out)
{
    double sum_free = 0.0, obj = 0.0, ub = __builtin_inf(), lb = -__builtin_inf();
    int n_free = 0;
    for (int t = 0; t < n; t++) {
        const double a = alpha[t], yg = y[t] > 0 ? g[t] : -g[t];
        if (a > 0.0 && a < C) { sum_free = sum_free + yg; n_free++; }
        else if ((y[t] > 0) == (a <= 0.0)) { if (yg < ub) ub = yg; }
        else { if (yg > lb) lb = yg; }
        obj = obj + a * (g[t] - 1.0);
    }
    out->rho = n_free > 0 ? sum_free / (double)n_free : (ub + lb) / 2.0;
    out->objective = obj / 2.0;
}

/* w[k] = sum_t (y_t alpha_t) x_t[k] in fp64 in ascending t, rounded once to f32 (cv::ml::SVM's compression of a linear model's support
 * vectors); alpha = 0 adds nothing and is skipped.  idx: the pair's dataset rows. */
SVM_FN float svm_weight(const uint8_t* samples, const int32_t* idx, const int8_t* y, const double* alpha, int n, int k)
{
    double s = 0.0;
    for (int t = 0; t < n; t++) {
        const double a = alpha[t];
        if (a > 0.0) s = s + (y[t] > 0 ? a : -a) * (double)samples[(int64_t)idx[t] * SVM_NFEAT + k];
    }
    return (float)s;
}

/* ---- the sequential form of one pair problem ----
 * G: [N][N]; idx, y: the pair's n rows; alpha, g: n doubles each, left as the solver leaves them */
SVM_FN void svm_solve_seq(const int32_t* G, int N, const int32_t* idx, const int8_t* y, int n, double C, double eps, int max_iter,
                          double* alpha, double* g, SvmPairOut* out)
{
    for (int t = 0; t < n; t++) { alpha[t] = 0.0; g[t] = -1.0; }
    int it = 0, conv = 0;
    for (;;) {
        SvmSel s;
        svm_sel_init(&s);
        for (int t = 0; t < n; t++) svm_sel_offer(&s, t, y[t], alpha[t], g[t], C);
        if (svm_sel_done(&s, eps)) { conv = 1; break; }
        if (it >= max_iter) break;
        const int32_t* gi = G + (int64_t)idx[s.i] * N;
        const int32_t* gj = G + (int64_t)idx[s.j] * N;
        const SvmStep st = svm_step(y[s.i], y[s.j], alpha[s.i], alpha[s.j], s.m, s.M, svm_eta_int(gi[idx[s.i]], gj[idx[s.j]], gi[idx[s.j]]), C);
        for (int t = 0; t < n; t++) g[t] = svm_grad(g[t], svm_q(y[t], y[s.i], gi[idx[t]]), st.dai, svm_q(y[t], y[s.j], gj[idx[t]]), st.daj);
        alpha[s.i] = st.ai;
        alpha[s.j] = st.aj;
        it++;
    }
    svm_finish(y, alpha, g, n, C, out);
    out->iterations = it;
    out->converged = conv;
}

/* ---- predict: device_classify.h:259-285 restated ----
 * one decision function: quads of f32 products summed left to right in f32, the quads accumulated in fp64 in feature order, the sum
 * rounded to f32 (cv's kernel value), then -rho + it in fp64 */
SVM_FN double svm_decide(const float* w, const float* feat, double rho)
{
    double s = 0;
    for (int k = 0; k < SVM_NFEAT; k += 4) s += w[k] * feat[k] + w[k + 1] * feat[k + 1] + w[k + 2] * feat[k + 2] + w[k + 3] * feat[k + 3];
    const float kval = (float)(s * 1.0 + 0.0);
    return -rho + 1.0 * kval;
}
/* the vote: pair (i < j, row-major) votes i when its sum is > 0, else j; the first maximum wins.  Eight 4-bit counters of one word. */
SVM_FN int svm_vote(const double* sums, int n_class)
{
    uint32_t votes = 0;
    int df = 0;
    for (int i = 0; i < n_class; i++)
        for (int j = i + 1; j < n_class; j++, df++) votes += 1u << (4 * (sums[df] > 0 ? i : j));
    int best = 0, bv = (int)(votes & 15u);
    for (int q = 1; q < n_class; q++) {
        const int vq = (int)((votes >> (4 * q)) & 15u);
        if (vq > bv) { best = q; bv = vq; }
    }
    return best;
}
/* the class INDEX of one row (sequential form); sums: 28 doubles, feat: 1200 floats of scratch */
SVM_FN int svm_predict_row(const float* weights, const double* rho, int n_class, const uint8_t* row, float* feat, double* sums)
{
    const int n_df = n_class * (n_class - 1) / 2;
    for (int k = 0; k < SVM_NFEAT; k++) feat[k] = (float)row[k];
    for (int d = 0; d < n_df; d++) sums[d] = svm_decide(weights + (int64_t)d * SVM_NFEAT, feat, rho[d]);
    return svm_vote(sums, n_class);
}

#endif
