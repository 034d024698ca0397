"""The seeded, tiny case list of the icon classifier's trainer (tests/test_svm_cpu.py, tests/test_gpu_svm.py, tests/test_svm_sanitized.py).
Each case names the branches of DESIGN.md 4l it is there for (`wants`); check(case) asserts them on the restatement ALONE
(tests/svm_train_ref.py counts the branches a run takes), so a case cannot silently stop covering its branch.  reference(case) is
computed once per process and shared."""
import functools

import numpy as np

import svm_train_ref as R

NFEAT = 1200
GRAM_TILE = 64


def _sparse_rows(rng, n, d, hi, shift=0):
    """rows whose first d features are small integers (kernel values stay small, so alphas reach the costs of a grid); the rest zero"""
    x = np.zeros((n, NFEAT), np.uint8)
    x[:, :d] = rng.randint(0, hi + 1, (n, d)) + shift
    return x


def _icons(rng, n_class, per_class, noise):
    """seeded prototype icons plus noise, classes in order"""
    protos = rng.randint(0, 256, (n_class, NFEAT))
    rows = [np.clip(protos[c] + rng.randint(-noise, noise + 1, (per_class, NFEAT)), 0, 255) for c in range(n_class)]
    return np.concatenate(rows).astype(np.uint8), np.repeat(np.arange(n_class), per_class).astype(np.int32)


def _pair(n, seed, overlap):
    """two classes, n rows in all, interleaved in dataset order; overlap: the classes share their distribution"""
    rng = np.random.RandomState(seed)
    resp = (np.arange(n) % 2).astype(np.int32) * 3 + 4               # responses 4 and 7: labels are not class indices
    x = _sparse_rows(rng, n, 6, 3)
    if not overlap:
        x[resp == 7, :6] += 5
    return x, resp


def _plain(c, **kw):
    return dict({"eps": 1e-3, "max_iter": 1000, "k_fold": 1, "c_grid": [c]}, **kw)


def build():
    cases = []

    def add(name, samples, responses, params, wants, perm=None, **checks):
        cases.append({"name": name, "samples": np.ascontiguousarray(samples, np.uint8), "responses": np.ascontiguousarray(responses, np.int32),
                      "perm": perm, "params": params, "wants": wants, "checks": checks})

    # pair sizes 2, 63, 64, 65 and 300 (more than one pass of a 256-thread workgroup); 63, 65, 300 are no multiple of the Gram tile
    for n in (2, 63, 64, 65, 300):
        x, r = _pair(n, 100 + n, overlap=n in (64, 300))
        add("pair_%d" % n, x, r, _plain(0.5), ["cut0"] if n == 2 else ["cut0", "selection_tie"], pair_size=n, off_tile=n in (63, 65, 300))
    # all-255 rows: the Gram maximum
    x, r = _icons(np.random.RandomState(7), 2, 3, 20)
    x[0] = x[4] = 255
    add("all_255", x, r, _plain(0.1), ["converged"], gram_max=True)
    # all-zero rows in both classes: the curvature of the first step is 0
    rng = np.random.RandomState(8)
    x = _sparse_rows(rng, 6, 6, 3, shift=1)
    x[0] = x[3] = 0
    add("all_zero", x, [0, 0, 0, 1, 1, 1], _plain(0.5), ["eta_floor"], zero_rows=True)
    # duplicated rows within a class: ties beyond the first selection
    x, r = _pair(12, 9, overlap=True)
    x[2], x[4], x[5] = x[0], x[0], x[1]
    add("duplicates", x, r, _plain(0.5), ["selection_tie"], min_ties=3)
    # the same row in both classes at a small C: both alphas clip at C, no free alpha -> the rho midpoint
    x = _sparse_rows(np.random.RandomState(10), 1, 6, 3, shift=1)
    add("same_row", np.concatenate([x, x]), [1, 2], _plain(0.01), ["eta_floor", "cut1", "two_at_C", "rho_midpoint"])
    # a separable set that converges well before max_iter (in less than half of it)
    x, r = _icons(np.random.RandomState(11), 2, 8, 30)
    add("separable", x, r, _plain(0.1), ["converged", "rho_free"], converges_before=500)
    # an overlapping set cut off at max_iter = 7
    x, r = _pair(40, 12, overlap=True)
    add("cut_off", x, r, _plain(0.5, max_iter=7), ["max_iter"], cut_off=True)
    # 8 classes through trainAuto; k_fold = 3 does not divide N = 40; the two grid entries tie on error and the earlier one wins
    x, r = _icons(np.random.RandomState(13), 8, 5, 40)
    add("eight_auto", x, r * 10 - 30, {"eps": 1e-3, "max_iter": 1000, "k_fold": 3, "c_grid": [0.1, 0.5]}, ["grid_tie", "converged"],
        perm=np.random.RandomState(14).permutation(40).astype(np.int32), n_class=8, fold_remainder=True, best_index=0)
    # 2 classes through trainAuto on overlapping rows: the grid entries differ in error
    x, r = _pair(45, 15, overlap=False)
    x[::7, :6] = 4
    add("two_auto", x, r, {"eps": 1e-3, "max_iter": 200, "k_fold": 4, "c_grid": [1e-4, 0.5, 2.5]}, ["cut1"],
        perm=np.random.RandomState(16).permutation(45).astype(np.int32), n_class=2, fold_remainder=True)
    return cases


CASES = build()
NAMES = [c["name"] for c in CASES]


def by_name(name):
    return CASES[NAMES.index(name)]


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = by_name(name)
    R.BRANCHES.clear()
    out = R.train_auto(c["samples"], c["responses"], c["perm"], **c["params"])
    return out, dict(R.BRANCHES)


def reference(case):
    """the restatement's result of the case (shared: do not modify)"""
    return _reference(case["name"])[0]


def check(case):
    """the case covers what it is for -- asserted on the restatement alone"""
    ref, br = _reference(case["name"])
    k = case["checks"]
    for w in case["wants"]:
        assert br.get(w, 0) > 0, (case["name"], w, br)
    n = len(case["samples"])
    if "pair_size" in k:
        assert len(ref["lists"][0]) == k["pair_size"] == n
    if k.get("off_tile"):
        assert n % GRAM_TILE != 0
    if k.get("gram_max"):
        assert ref["G"].max() == 1200 * 255 * 255 == 78030000
    if k.get("zero_rows"):
        cls = ref["cls"]
        assert any(not case["samples"][r].any() for r in np.flatnonzero(cls == 0)) and any(not case["samples"][r].any() for r in np.flatnonzero(cls == 1))
    if "min_ties" in k:
        assert br["selection_tie"] >= k["min_ties"]
    if "converges_before" in k:
        assert ref["converged"] == [1] and 0 < ref["iterations"][0] < k["converges_before"]
    if k.get("cut_off"):
        assert ref["converged"] == [0] and ref["iterations"] == [7]
    if "n_class" in k:
        assert len(ref["labels"]) == k["n_class"]
    if k.get("fold_remainder"):
        assert n % case["params"]["k_fold"] != 0
    if "best_index" in k:
        assert ref["best_index"] == k["best_index"] and ref["cv_errors"].count(min(ref["cv_errors"])) > 1
    if case["name"] == "two_auto":
        assert len(set(ref["cv_errors"])) > 1
