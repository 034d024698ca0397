"""The icon classifier's trainer on the device (rmcv_svm_gram, rmcv_svm_train, rmcv_svm_predict: k_svm.hip) against its
sequential form (rmcv_svm_*_host, which tests/test_svm_cpu.py holds to the restatement): the Gram matrix as integers; every output of
every case of tests/svm_cases.py bit for bit, alphas included; rmcv_svm_predict against the classifier stage on a synthetic frame's own
icons; and the route rows -> Dataset.sample -> train_auto -> Model.load_into -> held-out accuracy against the restatement's count."""
import numpy as np
import pytest

import svm_cases as K
import svm_train_ref as R
from rmcv_amd import svm, synth

pytestmark = pytest.mark.gpu


def bits(a, dtype):
    return np.ascontiguousarray(a, dtype).tobytes()


def test_gram_equals_the_host_gram(ctx):
    rng = np.random.RandomState(31)
    full = rng.randint(0, 256, (130, 1200)).astype(np.uint8)     # three tiles a side, the last one ragged
    full[7] = full[129] = 255                                    # the maximum, in the last tile too
    for rows in (K.by_name("pair_2")["samples"], K.by_name("pair_63")["samples"], K.by_name("pair_64")["samples"], K.by_name("pair_65")["samples"], full,
                 K.by_name("pair_300")["samples"]):
        got = svm.gram(rows, ctx=ctx)
        assert got.dtype == np.int32 and np.array_equal(got, svm.gram(rows))
    assert svm.gram(full, ctx=ctx).max() == 78030000
    ctx.check_guards()


@pytest.mark.parametrize("name", K.NAMES)
def test_train_equals_train_host_bit_for_bit(ctx, name):
    case = K.by_name(name)
    host = svm.train_auto(case["samples"], case["responses"], case["perm"], alphas=True, **case["params"])
    dev = svm.train_auto(case["samples"], case["responses"], case["perm"], ctx=ctx, alphas=True, **case["params"])
    assert dev.labels.tolist() == host.labels.tolist()
    assert bits(dev.report["alpha"], np.float64) == bits(host.report["alpha"], np.float64)
    assert bits(dev.rho, np.float64) == bits(host.rho, np.float64)
    assert bits(dev.weights, np.float32) == bits(host.weights, np.float32)
    assert dev.report["iterations"].tolist() == host.report["iterations"].tolist() and dev.report["converged"].tolist() == host.report["converged"].tolist()
    assert bits(dev.report["objective"], np.float64) == bits(host.report["objective"], np.float64)
    assert dev.report["cv_errors"] == host.report["cv_errors"] and dev.report["best_index"] == host.report["best_index"] and dev.report["best_c"] == host.report["best_c"]


def test_train_at_the_pair_limit(ctx):
    """2048 rows in two classes: a pair problem that fills the workgroup's LDS tables to their last entry (eight passes of the 256 threads),
    a Gram matrix of 32 x 32 full tiles; cut off after 60 iterations, which is all that bit-equality with the sequential form needs"""
    from rmcv_amd import abi
    n = abi.SVM_MAX_PAIR_SAMPLES
    rng = np.random.RandomState(51)
    rows = np.zeros((n, 1200), np.uint8)
    rows[:, :8] = rng.randint(0, 4, (n, 8))
    rows[:, 1199] = rng.randint(0, 256, n)                        # the last feature takes part
    resp = (rng.randint(0, 2, n) * 5).astype(np.int32)
    resp[-1], resp[0] = 5, 0
    params = {"k_fold": 1, "c_grid": [0.5], "max_iter": 60}
    host = svm.train_auto(rows, resp, alphas=True, **params)
    dev = svm.train_auto(rows, resp, ctx=ctx, alphas=True, **params)
    assert host.report["iterations"].tolist() == [60] and np.count_nonzero(host.report["alpha"][0]) > 2
    assert bits(dev.report["alpha"], np.float64) == bits(host.report["alpha"], np.float64) and bits(dev.rho, np.float64) == bits(host.rho, np.float64)
    assert bits(dev.weights, np.float32) == bits(host.weights, np.float32) and bits(dev.report["objective"], np.float64) == bits(host.report["objective"], np.float64)
    assert dev.report["iterations"].tolist() == [60] and dev.report["converged"].tolist() == [0]
    x = rows.astype(np.float64)
    assert np.array_equal(svm.gram(rows, ctx=ctx), (x @ x.T).astype(np.int32))      # exact in fp64: every entry is an integer below 2^53
    ctx.check_guards()


def test_refusals_come_before_any_gpu_work(ctx):
    from rmcv_amd import RmcvError, abi
    rows = np.zeros((12, 1200), np.uint8)
    with pytest.raises(RmcvError) as e:
        ctx.svm_train(rows, np.zeros(12))
    assert e.value.code == abi.ERR_BAD_ARG and "fewer than 2 classes" in str(e.value)
    with pytest.raises(RmcvError) as e:
        ctx.svm_train(rows, np.arange(12) % 3, perm=[0] * 12)
    assert e.value.code == abi.ERR_BAD_ARG and "not a permutation" in str(e.value)


def test_predict_equals_the_classifier_stage_on_a_frames_icons(ctx):
    """rmcv_svm_predict restates device_classify.h's decision rule: on the icons rmcv_classify_armours hands out it returns the identities
    that call returned"""
    model = synth.svm_weights()
    ctx.svm_load(*model)
    frame = synth.frame(3, 1920, 1200)
    arm, offs = ctx.detect_batch(frame[None])
    assert len(arm) >= 2
    identity, _, icons = ctx.classify_armours(frame, arm)
    rows = icons.reshape(len(arm), 1200)
    assert ctx.svm_predict(rows).tolist() == identity.tolist()
    weights, rho, labels = model
    assert svm.Model(weights, rho, labels).predict(rows).tolist() == identity.tolist()      # ... and so does the sequential form
    assert ctx.svm_predict(rows[:0]).tolist() == []


def test_end_to_end_rows_to_loaded_model(ctx, tmp_path):
    rng = np.random.RandomState(41)
    protos = rng.randint(0, 256, (7, 1200))
    data = svm.Dataset(["1", "2", "3", "4", "5", "Sentry", "Negtive"])
    for k in range(7):
        data.add(k, np.clip(protos[k] + rng.randint(-110, 111, (40, 1200)), 0, 255))
    train, held = data.sample(0.6, seed=42)
    samples, responses = train.format_data()
    held_rows, held_resp = held.format_data()
    assert len(samples) == 7 * 24 and len(held_rows) == 7 * 16
    perm = np.random.RandomState(43).permutation(len(samples)).astype(np.int32)
    params = {"k_fold": 4, "c_grid": [0.1, 2.5]}
    model = ctx.svm_train(samples, responses, perm, **params)
    path = str(tmp_path / "model.rmcvsvm")
    model.save(path)
    svm.Model.load(path).load_into(ctx)
    got = ctx.svm_predict(held_rows)
    # the restatement: its own training, its own predict
    ref = R.train_auto(samples, responses, perm, **params)
    want = np.array(ref["labels"])[R.predict(ref["W"], ref["rho"], 7, held_rows)]
    ref_correct = int(np.count_nonzero(want == held_resp))
    assert ref_correct > len(held_rows) / 7                       # above chance, asserted on the restatement
    assert int(np.count_nonzero(got == held_resp)) == ref_correct and got.tolist() == want.tolist()
    assert model.report["cv_errors"] == ref["cv_errors"] and model.report["best_index"] == ref["best_index"]
