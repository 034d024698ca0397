"""The sequential form of the icon classifier's trainer (rmcv_svm_train_host, rmcv_svm_gram_host, rmcv_svm_predict_host: DESIGN.md 4l)
against the independent restatement tests/svm_train_ref.py, bit for bit, over tests/svm_cases.py; an optimality certificate that does
not depend on the algorithm; every refusal; and the Python layer (Dataset, Model).  No GPU."""
import numpy as np
import pytest

import svm_cases as K
import svm_train_ref as R
from rmcv_amd import RmcvError, abi, svm


def bits(a, dtype):
    return np.ascontiguousarray(a, dtype).tobytes()


@pytest.mark.parametrize("name", K.NAMES)
def test_case_covers_its_branches(name):
    K.check(K.by_name(name))


@pytest.mark.parametrize("name", K.NAMES)
def test_train_host_equals_the_restatement_bit_for_bit(name):
    case = K.by_name(name)
    ref = K.reference(case)
    assert np.array_equal(svm.gram(case["samples"]), ref["G"])
    m = svm.train_auto(case["samples"], case["responses"], case["perm"], alphas=True, **case["params"])
    assert m.labels.tolist() == ref["labels"]
    assert bits(m.report["alpha"], np.float64) == bits(ref["alpha"], np.float64)
    assert bits(m.rho, np.float64) == bits(ref["rho"], np.float64)
    assert bits(m.weights, np.float32) == bits(ref["W"], np.float32)
    assert m.report["iterations"].tolist() == ref["iterations"] and m.report["converged"].tolist() == ref["converged"]
    assert bits(m.report["objective"], np.float64) == bits(ref["objective"], np.float64)
    assert m.report["cv_errors"] == ref["cv_errors"] and m.report["best_index"] == ref["best_index"] and m.report["best_c"] == ref["best_c"]


def recomputed_gradient(G, rows, y, alpha):
    """g = Q alpha - e from scratch (numpy's own summation order)"""
    Q = (np.outer(y, y) * G[np.ix_(rows, rows)]).astype(np.float64)
    return Q @ alpha - 1.0


def converged_problems():
    for case in K.CASES:
        ref = K.reference(case)
        for d, (res, rows) in enumerate(zip(ref["results"], ref["lists"])):
            if res["converged"]:
                yield case, ref, d, res, rows, np.where(ref["cls"][rows] == R.pairs(len(ref["labels"]))[d][0], 1.0, -1.0)


def test_optimality_certificate():
    """Independent of the algorithm: for every converged pair problem of the case list, the LIBRARY's alphas satisfy the stopping rule on a
    gradient recomputed from scratch, g = Q alpha - e: max over Up of -y g minus min over Low of -y g < eps + slack.  slack is 4 x the
    largest |incremental g - recomputed g| of the restatement over these problems (the recomputation sums in another order); measured:
    8.84e-10 (kernel values reach 7.8e7, and a gradient is a few hundred rounded updates of that size).  It is computed here, not fixed;
    the assertion on it only says that the certificate means something: the slack stays below a tenth of eps."""
    worst = max(float(np.abs(res["g"] - recomputed_gradient(ref["G"], rows, y, res["alpha"])).max()) for _, ref, _, res, rows, y in converged_problems())
    print("largest |incremental g - recomputed g| of the restatement: %.3g" % worst)
    assert 4 * worst < 1e-3 / 10
    slack, seen = 4 * worst, 0
    models = {}
    for case, ref, d, res, rows, y in converged_problems():
        if case["name"] not in models:
            models[case["name"]] = svm.train_auto(case["samples"], case["responses"], case["perm"], alphas=True, **case["params"])
        m = models[case["name"]]
        C, alpha = m.report["best_c"], m.report["alpha"][d][rows]
        assert (alpha >= 0).all() and (alpha <= C).all()
        g = recomputed_gradient(ref["G"], rows, y, alpha)
        v = -y * g
        up, low = ((y > 0) & (alpha < C)) | ((y < 0) & (alpha > 0)), ((y > 0) & (alpha > 0)) | ((y < 0) & (alpha < C))
        if up.any() and low.any():
            assert v[up].max() - v[low].min() < case["params"]["eps"] + slack, (case["name"], d)
            seen += 1
    assert seen >= 30


def test_predict_host_equals_the_restatement_on_held_out_rows():
    case = K.by_name("eight_auto")
    ref = K.reference(case)
    rng = np.random.RandomState(21)
    held = np.clip(case["samples"][rng.randint(0, len(case["samples"]), 60)].astype(np.int64) + rng.randint(-90, 91, (60, 1200)), 0, 255).astype(np.uint8)
    want = np.array(ref["labels"])[R.predict(ref["W"], ref["rho"], len(ref["labels"]), held)]
    m = svm.Model(ref["W"], ref["rho"], ref["labels"])
    assert m.predict(held).tolist() == want.tolist()
    assert len(set(want.tolist())) >= 4                      # the rows do not all fall into one class
    assert m.predict(held[:0]).tolist() == []


def refused(samples, responses, perm=None, **params):
    with pytest.raises(RmcvError) as e:
        svm.train_auto(samples, responses, perm, **params)
    assert e.value.code == abi.ERR_BAD_ARG
    return str(e.value)


def test_every_refusal_refuses():
    rows = np.zeros((12, 1200), np.uint8)
    resp = np.arange(12) % 3
    assert "fewer than 2 classes" in refused(rows, np.zeros(12))
    assert "more than 8 classes" in refused(rows, np.arange(12) % 9)
    assert "fewer than 2 rows" in refused(rows[:1], [0])
    assert "not a permutation" in refused(rows, resp, perm=[0] * 12)
    assert "not a permutation" in refused(rows, resp, perm=list(range(1, 13)))
    assert "not a permutation" in refused(rows, resp, perm=[-1] + list(range(1, 12)))
    # a class with one row, leave-one-out: the fold that tests the row trains without its class
    assert "lacks a class" in refused(rows, [0] * 6 + [1] * 5 + [2], k_fold=12)
    assert "RMCV_SVM_MAX_SAMPLES" in refused(np.zeros((abi.SVM_MAX_SAMPLES + 1, 1200), np.uint8), np.arange(abi.SVM_MAX_SAMPLES + 1) % 8)
    assert "RMCV_SVM_MAX_PAIR_SAMPLES" in refused(np.zeros((abi.SVM_MAX_PAIR_SAMPLES + 1, 1200), np.uint8), np.arange(abi.SVM_MAX_PAIR_SAMPLES + 1) % 2)
    assert "eps" in refused(rows, resp, eps=-1.0) and "eps" in refused(rows, resp, eps=float("nan"))
    assert "max_iter" in refused(rows, resp, max_iter=0)
    assert "folds" in refused(rows, resp, k_fold=abi.SVM_MAX_FOLDS + 1)
    assert "every C" in refused(rows, resp, c_grid=[0.1, 0.0]) and "every C" in refused(rows, resp, c_grid=[float("inf")])
    # the same rows are accepted once nothing is wrong (k_fold <= 1 or one grid entry: plain training, no search)
    m = svm.train_auto(rows, resp, k_fold=12, c_grid=[0.1])
    assert m.report["cv_errors"] == [-1] and m.report["best_index"] == 0
    L = abi.lib()
    assert L.rmcv_svm_train_host(None, None, 12, None, None, None, None, None, None, None) == abi.ERR_BAD_ARG
    assert L.rmcv_svm_gram_host(None, 1, None) == abi.ERR_BAD_ARG and L.rmcv_svm_gram_host(abi.ptr(rows), 0, abi.ptr(rows)) == abi.ERR_BAD_ARG
    assert L.rmcv_svm_predict_host(None, None, None, 2, None, 0, None) == abi.ERR_BAD_ARG
    # without a context the device entry points answer at once (no CPU path behind them)
    assert L.rmcv_svm_train(None, abi.ptr(rows), abi.ptr(rows), 12, None, None, abi.ptr(rows), abi.ptr(rows), abi.ptr(rows), abi.ptr(rows), None) == abi.ERR_BAD_ARG
    assert L.rmcv_svm_gram(None, abi.ptr(rows), 12, abi.ptr(rows)) == abi.ERR_BAD_ARG and L.rmcv_svm_predict(None, abi.ptr(rows), 1, abi.ptr(rows)) == abi.ERR_BAD_ARG


def test_defaults_are_the_reference_criteria_and_opencvs_grid():
    p = svm.default_train_params()
    d = R.default_params()
    assert (p.eps, p.max_iter, p.k_fold, p.n_c) == (1e-3, 1000, 10, 6) == (d["eps"], d["max_iter"], d["k_fold"], len(d["c_grid"]))
    assert list(p.c_grid[:6]) == d["c_grid"] and abs(p.c_grid[5] - 312.5) < 1e-12


def test_dataset_and_model_container(tmp_path):
    rng = np.random.RandomState(3)
    data = svm.Dataset(["a", "b", "c"])
    for k, m in enumerate((10, 7, 5)):
        data.add(k, rng.randint(0, 256, (m, 1200)))
    head, tail = data.sample(0.6, seed=5)
    assert [len(head[k]) for k in range(3)] == [6, 4, 3] and [len(tail[k]) for k in range(3)] == [4, 3, 2]      # int(float32(m) * float32(0.6))
    for k in range(3):                                                                                         # a split of the class's rows
        assert sorted(map(bytes, np.concatenate([head[k], tail[k]]))) == sorted(map(bytes, data[k]))
    again, _ = data.sample(0.6, seed=5)
    other, _ = data.sample(0.6, seed=6)
    assert all(np.array_equal(head[k], again[k]) for k in range(3)) and not all(np.array_equal(head[k], other[k]) for k in range(3))
    samples, responses = head.format_data()
    assert samples.shape == (13, 1200) and responses.tolist() == [0] * 6 + [1] * 4 + [2] * 3
    m = svm.train_auto(samples, responses, k_fold=1)
    path = str(tmp_path / "model.rmcvsvm")
    m.save(path)
    back = svm.Model.load(path)
    assert bits(back.weights, np.float32) == bits(m.weights, np.float32) and bits(back.rho, np.float64) == bits(m.rho, np.float64) and back.labels.tolist() == [0, 1, 2]
    open(path, "ab").write(b"x")
    with pytest.raises(RmcvError):
        svm.Model.load(path)
