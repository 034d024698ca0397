// TEST-ONLY stand-alone program around the host path of the icon classifier's trainer (rmcv_amd/csrc/svm_plan.h: svm_train_seq, over
// device_svm.h), for a sanitizer build (tests/test_svm_sanitized.py: -fsanitize=address,undefined; no GPU, nothing loaded into python).
// Every table is a heap block of exactly its size, so a row or a decision function too far shows.
//   svm_san_main IN OUT
// IN : int32 n, int32 has_perm, rmcv_svm_train_params, uint8 samples[n][1200], int32 responses[n], int32 perm[n] if has_perm
// OUT: int32 rc; then, if rc == 0: int32 n_class, int32 labels[n_class], float weights[n_df][1200], double rho[n_df], int32 best_index,
//      double best_c, int32 cv_errors[n_c], int32 iterations[n_df], int32 converged[n_df], double objective[n_df], double alpha[n_df][n],
//      int32 held_out[n] (rmcv_svm_predict_host's rule on the training rows themselves)
#include <cstdio>
#include <cstdlib>

#include "../rmcv_amd/csrc/svm_plan.h"

template <typename T> static T* block(size_t n) { return static_cast<T*>(std::calloc(n ? n : 1, sizeof(T))); }
template <typename T> static void get(std::FILE* f, T* p, size_t n) { if (std::fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); } }
template <typename T> static void put(std::FILE* f, const T* p, size_t n) { if (std::fwrite(p, sizeof(T), n, f) != n) std::exit(3); }

int main(int argc, char** argv)
{
    if (argc != 3) return 1;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int32_t head[2];
    get(in, head, 2);
    const size_t n = (size_t)head[0];
    rmcv_svm_train_params p;
    get(in, &p, 1);
    uint8_t* samples = block<uint8_t>(n * SVM_NFEAT);
    int32_t* responses = block<int32_t>(n);
    int32_t* perm = block<int32_t>(n);
    get(in, samples, n * SVM_NFEAT);
    get(in, responses, n);
    if (head[1]) get(in, perm, n);
    // the class count first (a plan of its own), so that every output block has exactly its size
    rmcv::SvmPlan pl;
    const char* why = rmcv::svm_plan_build(pl, responses, (int)n, head[1] ? perm : nullptr, p);
    int32_t rc = why ? RMCV_ERR_BAD_ARG : RMCV_OK;
    if (!why) {
        const size_t n_df = (size_t)pl.n_df;
        float* weights = block<float>(n_df * SVM_NFEAT);
        double* rho = block<double>(n_df);
        int32_t* labels = block<int32_t>((size_t)pl.n_class);
        double* alpha = block<double>(n_df * n);
        int32_t n_class = 0;
        rmcv_svm_train_report rep;
        rep.alpha_out = alpha;
        why = rmcv::svm_train_seq(samples, responses, (int)n, head[1] ? perm : nullptr, p, weights, rho, labels, &n_class, &rep);
        rc = why ? RMCV_ERR_BAD_ARG : RMCV_OK;
        put(out, &rc, 1);
        if (!why) {
            put(out, &n_class, 1);
            put(out, labels, (size_t)n_class);
            put(out, weights, n_df * SVM_NFEAT);
            put(out, rho, n_df);
            put(out, &rep.best_index, 1);
            put(out, &rep.best_c, 1);
            put(out, rep.cv_errors, (size_t)p.n_c);
            put(out, rep.iterations, n_df);
            put(out, rep.converged, n_df);
            put(out, rep.objective, n_df);
            put(out, alpha, n_df * n);
            int32_t* held = block<int32_t>(n);
            float* feat = block<float>(SVM_NFEAT);
            double* sums = block<double>(n_df);
            for (size_t r = 0; r < n; r++) held[r] = labels[svm_predict_row(weights, rho, n_class, samples + r * SVM_NFEAT, feat, sums)];
            put(out, held, n);
            std::free(held); std::free(feat); std::free(sums);
        }
        std::free(weights); std::free(rho); std::free(labels); std::free(alpha);
    } else {
        std::fprintf(stderr, "%s\n", why);
        put(out, &rc, 1);
    }
    std::free(samples); std::free(responses); std::free(perm);
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 3;
}
