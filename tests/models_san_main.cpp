// models_san_main.cpp -- rmcv_amd/csrc/model_plan.h (and run_steps of bind_plan.h) compiled for the host, as a stand-alone program:
//   models_san_main <case file> <output file>
// Reads the tables and index lists of tests/model_cases.py, holds every array in a heap block of EXACTLY its size (so that a read or
// write past a model's decision functions or labels, or past a table's last entry, is one AddressSanitizer sees), packs or refuses them,
// writes the packed tables to the output file and prints one line per answer.  tests/test_model_plan.py builds it plain,
// tests/test_models_sanitized.py with -fsanitize=address,undefined; both compare with tests/model_ref.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../rmcv_amd/csrc/bind_plan.h"
#include "../rmcv_amd/csrc/model_plan.h"

using namespace rmcv;

static FILE* g_in;
template <typename T>
static std::unique_ptr<T[]> take(size_t n)
{
    std::unique_ptr<T[]> p(new T[n ? n : 1]);
    if (n && fread(p.get(), sizeof(T), n, g_in) != n) { fprintf(stderr, "case file truncated\n"); exit(2); }
    return p;
}
static int32_t take_int()
{
    int32_t v;
    if (fread(&v, 4, 1, g_in) != 1) { fprintf(stderr, "case file truncated\n"); exit(2); }
    return v;
}

static bool same_steps(const RunSteps& a, const RunSteps& b, bool but_identity)
{
    const bool rest = a.refusal == b.refusal && a.status_clear == b.status_clear && a.enhance_tables == b.enhance_tables && a.window_origins == b.window_origins &&
                      a.frame_keys == b.frame_keys && a.binary == b.binary && a.image == b.image && a.sparse == b.sparse && a.sparse_pairs == b.sparse_pairs &&
                      a.contours == b.contours && a.match == b.match && a.match_pairs == b.match_pairs && a.blobs_armours == b.blobs_armours && a.blobs == b.blobs &&
                      a.armours == b.armours && a.pnp == b.pnp;
    return rest && (but_identity || (a.sparse_identity == b.sparse_identity && a.classify == b.classify));
}

int main(int argc, char** argv)
{
    if (argc != 3 || !(g_in = fopen(argv[1], "rb"))) return 2;
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    char msg[200];
    // ---- the tables: refused with a message, or packed
    const int n_tables = take_int();
    for (int t = 0; t < n_tables; t++) {
        const int n_models = take_int(), null_table = take_int(), given = take_int();
        std::vector<std::unique_ptr<float[]>> w;
        std::vector<std::unique_ptr<double[]>> r;
        std::vector<std::unique_ptr<int32_t[]>> l;
        std::unique_ptr<rmcv_svm_model[]> models(new rmcv_svm_model[given ? given : 1]);
        for (int m = 0; m < given; m++) {
            const int n_class = take_int(), mask = take_int(), d = take_int();
            w.push_back(take<float>((size_t)d * MODEL_NFEAT));
            r.push_back(take<double>((size_t)d));
            l.push_back(take<int32_t>(d ? (size_t)n_class : 0));
            models[m].weights = (mask & 1) ? nullptr : w.back().get();
            models[m].rho = (mask & 2) ? nullptr : r.back().get();
            models[m].labels = (mask & 4) ? nullptr : l.back().get();
            models[m].n_class = n_class;
            models[m].reserved = 0;
        }
        const char* no = models_refusal(null_table ? nullptr : models.get(), n_models, msg);
        if (no) {
            printf("T %d : %s\n", t, no);
            continue;
        }
        std::unique_ptr<SvmModelEntry[]> table(new SvmModelEntry[n_models]);
        for (int m = 0; m < n_models; m++) model_pack(models[m], &table[m]);
        fwrite(table.get(), sizeof(SvmModelEntry), (size_t)n_models, out);
        printf("T %d : ok %zu\n", t, sizeof(SvmModelEntry) * (size_t)n_models);
    }
    // ---- the rule
    for (int n : {1, 2, 64})
        for (int64_t idx : {(int64_t)INT32_MIN, (int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)n - 1, (int64_t)n, (int64_t)INT32_MAX})
            printf("R %d %lld : %d\n", n, (long long)idx, (int)frame_model_eff((int32_t)idx, n));
    // ---- the host setter's indices
    const int n_setter = take_int();
    for (int i = 0; i < n_setter; i++) {
        const int n_models = take_int(), n_frames = take_int();
        const std::unique_ptr<int32_t[]> idx = take<int32_t>((size_t)n_frames);
        const char* no = frame_models_refusal(idx.get(), n_frames, n_models, msg);
        printf("F %d : %s\n", i, no ? no : "-");
    }
    // ---- the pipeline's submit
    for (int nf : {4, 5}) for (int tf : {4, 5}) for (int agree : {0, 1}) {
        const char* no = pipeline_models_refusal(nf, tf, agree != 0, msg);
        printf("P %d %d %d : %s\n", nf, tf, agree, no ? no : "-");
    }
    // ---- the run: models = 0 is the seven-argument call; models = 1 takes the classifier out of the fused kernel and launches it, nothing else
    int count = 0, off = 0;
    for (int stages = 1; stages <= 127; stages++) for (int m = 0; m < 64; m++) {
        const int fmt = (m >> 2) & 1 ? RMCV_BAYER_BG : RMCV_INPUT_BGR;
        const RunSteps a = run_steps(stages, m & 1, (m >> 1) & 1, fmt, (m >> 3) & 1, (m >> 4) & 1, (m >> 5) & 1);
        const RunSteps b = run_steps(stages, m & 1, (m >> 1) & 1, fmt, (m >> 3) & 1, (m >> 4) & 1, (m >> 5) & 1, 0);
        const RunSteps c = run_steps(stages, m & 1, (m >> 1) & 1, fmt, (m >> 3) & 1, (m >> 4) & 1, (m >> 5) & 1, 1);
        bool ok = same_steps(a, b, false);
        if (stages & RMCV_STAGE_IDENTITY) ok = ok && same_steps(a, c, true) && !c.sparse_identity && c.classify;
        else ok = ok && same_steps(a, c, false);
        count++;
        off += !ok;
    }
    printf("S %d %d\n", count, off);
    fclose(out);
    fclose(g_in);
    return 0;
}
