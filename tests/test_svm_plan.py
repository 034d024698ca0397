"""svm_plan.h (rmcv_amd/csrc) compiled with the host C++ compiler: what a training call decides before anything runs -- the class table,
the sample list of every (fold, pair) and final pair, the problem table (grid entry, fold, pair) -> list, cost and place of its alphas,
the workspace sizes, the limits and every refusal in its order -- against DESIGN.md 4l restated here."""
import os
import subprocess

import numpy as np
import pytest

import svm_train_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stdio.h>
#include <stdlib.h>
#include "rmcv_amd/csrc/svm_plan.h"
using namespace rmcv;
// stdin: n has_perm eps max_iter k_fold n_c c... responses... perm...
int main()
{
    int n, has_perm;
    rmcv_svm_train_params p;
    svm_default_params(&p);
    printf("D %g %d %d %d %.17g %.17g %.17g %.17g %.17g %.17g\n", p.eps, p.max_iter, p.k_fold, p.n_c, p.c_grid[0], p.c_grid[1], p.c_grid[2], p.c_grid[3], p.c_grid[4], p.c_grid[5]);
    printf("L %d %d %d %d %d %d %zu %zu\n", RMCV_SVM_MAX_SAMPLES, RMCV_SVM_MAX_PAIR_SAMPLES, RMCV_SVM_MAX_GRID, RMCV_SVM_MAX_DF, RMCV_SVM_MAX_FOLDS, SVM_GRAM_TILE, sizeof(SvmProblem), sizeof(SvmPairOut));
    while (scanf("%d %d %lf %d %d %d", &n, &has_perm, &p.eps, &p.max_iter, &p.k_fold, &p.n_c) == 6) {
        for (int k = 0; k < p.n_c && k < RMCV_SVM_MAX_GRID; k++) if (scanf("%lf", &p.c_grid[k]) != 1) return 2;
        std::vector<int32_t> resp(n > 0 ? n : 0), perm(n > 0 ? n : 0);
        for (int r = 0; r < n; r++) if (scanf("%d", &resp[r]) != 1) return 2;
        for (int r = 0; has_perm && r < n; r++) if (scanf("%d", &perm[r]) != 1) return 2;
        SvmPlan pl;
        const char* why = svm_plan_build(pl, resp.data(), n, has_perm ? perm.data() : nullptr, p);
        if (why) { printf("R %s\n", why); continue; }
        printf("P %d %d %d %d %d %lld %lld |", pl.n, pl.n_class, pl.n_df, pl.n_c, pl.k_fold, (long long)pl.search_alphas, (long long)pl.fin_alphas);
        for (int v : pl.labels) printf(" %d", v);
        printf(" |");
        for (int v : pl.cls) printf(" %d", v);
        printf(" |");
        for (int v : pl.fold_of) printf(" %d", v);
        printf("\n");
        for (int part = 0; part < 2; part++)
            for (const SvmProblem& q : part ? pl.fin : pl.search) {
                printf("Q %d %d %d %d %d %lld C=%.17g :", part, q.ci, q.cj, q.c_idx, q.fold, (long long)q.alpha_off, q.C);
                for (int t = 0; t < q.n; t++) printf(" %d", pl.lists[q.list_off + t]);
                printf("\n");
            }
        const SvmWorkspace w = svm_workspace(pl);
        printf("W %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", w.samples, w.gram, w.cls, w.lists, w.problems, w.alphas, w.weights, w.rho, w.outs, w.fold_of, w.pred, w.total());
    }
    const int32_t e1[4] = {3, 1, 1, 2}, e2[3] = {5, 5, 5};
    printf("B %d %d\n", svm_best_entry(e1, 4), svm_best_entry(e2, 3));
    return 0;
}
'''


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("svm_plan")
    src, exe = str(d / "svm_plan_main.cpp"), str(d / "svm_plan_main")
    open(src, "w").write(SRC)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-I", ROOT, src, "-o", exe], check=True)
    return exe


def question(responses, perm=None, eps=1e-3, max_iter=1000, k_fold=10, c_grid=(0.1, 0.5)):
    return {"responses": list(responses), "perm": None if perm is None else list(perm), "eps": eps, "max_iter": max_iter, "k_fold": k_fold, "c_grid": list(c_grid)}


def expected(q):
    """DESIGN.md 4l, refusals in the order the header makes them"""
    resp, perm, n, grid, K = q["responses"], q["perm"], len(q["responses"]), q["c_grid"], q["k_fold"]
    if not (q["eps"] >= 0 and np.isfinite(q["eps"])):
        return ["R svm train: eps must be finite and not negative"]
    if q["max_iter"] < 1:
        return ["R svm train: max_iter must be at least 1"]
    if K > 64:
        return ["R svm train: more than RMCV_SVM_MAX_FOLDS folds"]
    if not 1 <= len(grid) <= 16:
        return ["R svm train: n_c must be 1 .. RMCV_SVM_MAX_GRID"]
    if any(not (c > 0 and np.isfinite(c)) for c in grid):
        return ["R svm train: every C must be finite and positive"]
    if n < 2:
        return ["R svm train: fewer than 2 rows"]
    if n > 8192:
        return ["R svm train: more rows than RMCV_SVM_MAX_SAMPLES"]
    labels, cls = R.class_table(resp)
    if len(labels) < 2:
        return ["R svm train: fewer than 2 classes"]
    if len(labels) > 8:
        return ["R svm train: more than 8 classes"]
    if perm is not None and sorted(perm) != list(range(n)):
        return ["R svm train: perm is not a permutation of the rows"]
    pairs = R.pairs(len(labels))
    count = np.bincount(cls, minlength=len(labels))
    if any(count[i] + count[j] > 2048 for i, j in pairs):
        return ["R svm train: two classes have more rows together than RMCV_SVM_MAX_PAIR_SAMPLES"]
    search = K > 1 and len(grid) > 1
    fold_of, lines, lists_len, at = [], [], 0, 0
    if search:
        fold_of = np.zeros(n, int)
        for k, test in enumerate(R.folds(n, K, perm)):
            fold_of[test] = k
        for k in range(K):
            if any(np.count_nonzero((cls == c) & (fold_of != k)) == 0 for c in range(len(labels))):
                return ["R svm train: the training part of a fold lacks a class"]
        for ci, C in enumerate(grid):
            for k in range(K):
                for i, j in pairs:
                    rows = [r for r in range(n) if cls[r] in (i, j) and fold_of[r] != k]
                    lines.append("Q 0 %d %d %d %d %d C=%s : %s" % (i, j, ci, k, at, repr(float(C)), " ".join(map(str, rows))))
                    at += len(rows)
                    if ci == 0:
                        lists_len += len(rows)
    search_alphas, at = at, 0
    for i, j in pairs:
        rows = [r for r in range(n) if cls[r] in (i, j)]
        lines.append("Q 1 %d %d -1 -1 %d C=%s : %s" % (i, j, at, repr(float(grid[0])), " ".join(map(str, rows))))
        at += len(rows)
        lists_len += len(rows)
    n_df, n_c = len(pairs), len(grid) if search else 1
    probs = max(n_c * K * n_df if search else 0, n_df)
    sizes = [n * 1200, n * n * 4, n * 4, lists_len * 4, probs * 40, max(search_alphas, at) * 8, probs * 1200 * 4, probs * 8, probs * 24, n * 4, n_c * n * 4]
    head = "P %d %d %d %d %d %d %d | %s | %s | %s" % (n, len(labels), n_df, n_c, K if search else 0, search_alphas, at, " ".join(map(str, labels)), " ".join(map(str, cls)),
                                                   " ".join(map(str, fold_of)))
    return [head] + lines + ["W " + " ".join(map(str, sizes + [sum(sizes)]))]


def norm(line):
    """numbers as Python prints them, spaces collapsed"""
    out = []
    for tok in line.split():
        try:
            if tok.startswith("C="):
                tok = repr(float(tok[2:]))
            out.append(repr(float(tok)) if ("." in tok or "e" in tok or "inf" in tok or "nan" in tok) else tok)
        except ValueError:
            out.append(tok)
    return " ".join(out)


def test_plan_equals_the_restated_section(program):
    rng = np.random.RandomState(5)
    many = rng.randint(0, 3, 31) * 7 - 4
    qs = [
        question([5, 5, -2, 9, -2, 9, 5, 9, -2, 5, 9], k_fold=3),                                       # 3 classes, 11 rows, 3 folds: 3, 4, 4 rows
        question([5, 5, -2, 9, -2, 9, 5, 9, -2, 5, 9], perm=[10, 3, 7, 0, 1, 2, 9, 8, 4, 6, 5], k_fold=4),
        question(many, perm=rng.permutation(31), k_fold=10, c_grid=(0.1, 0.5, 2.5)),                     # folds of 3 and 4 rows
        question(many, k_fold=1), question(many, k_fold=0), question(many, k_fold=5, c_grid=(3.0,)),     # plain training, no search
        question(list(range(8)) * 2, k_fold=2), question(list(range(8)) * 2, k_fold=16),                 # 8 classes; leave-one-out with 2 rows per class
        question([1, 2], k_fold=1), question([1, 2], k_fold=2),                                          # 2 rows: a fold of 1 leaves a class out
        question(many, k_fold=40),                                                                        # more folds than rows: some are empty
        # refusals, each alone and in the header's order when several hold
        question(many, eps=-1e-9), question(many, eps=float("nan")), question(many, eps=float("inf")), question(many, max_iter=0), question(many, k_fold=65),
        question(many, c_grid=()), question(many, c_grid=[1.0] * 17), question(many, c_grid=(0.1, -1.0)), question(many, c_grid=(float("inf"), 1.0)),
        question([3]), question([]), question([0, 1] * 4097), question([4] * 9), question(list(range(9)) * 2),
        question(many, perm=list(range(30)) + [0]), question(many, perm=list(range(1, 32))), question(many, perm=[-1] + list(range(1, 31))),
        question([0] * 1025 + [1] * 1024 + [2] * 3, k_fold=1), question([0] * 1024 + [1] * 1024 + [2] * 3, k_fold=1),
        question([0, 0, 0, 1, 1, 2], k_fold=6), question([0, 0, 0, 1, 1, 2, 2], k_fold=7), question([0, 0, 0, 1, 1, 2], k_fold=2, perm=[5, 0, 3, 1, 2, 4]),
        question(many, eps=-1.0, max_iter=0, c_grid=()), question([1], k_fold=99),
    ]
    text = ""
    for q in qs:
        n = len(q["responses"])
        text += "%d %d %r %d %d %d %s\n%s\n%s\n" % (n, q["perm"] is not None, q["eps"], q["max_iter"], q["k_fold"], len(q["c_grid"]),
                                                   " ".join(repr(float(c)) for c in q["c_grid"][:16]), " ".join(map(str, q["responses"])),
                                                   " ".join(map(str, q["perm"] or [])))
    done = subprocess.run([program], input=text, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    got = [norm(line) for line in done.stdout.splitlines()]
    d = R.default_params()
    want = ["D 0.001 1000 10 6 " + " ".join(repr(c) for c in d["c_grid"]), "L 8192 2048 16 28 64 64 40 24"]
    kinds = set()
    for q in qs:
        e = expected(q)
        kinds.add(e[0] if e[0].startswith("R") else "P")
        want += e
    want.append("B 1 0")                                                                                  # the lowest error, the earlier entry on a tie
    want = [norm(line) for line in want]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    assert len(kinds) == 13                                                                               # every one of the 12 refusals was met, and plans too
