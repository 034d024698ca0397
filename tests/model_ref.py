"""rmcv_amd/csrc/model_plan.h restated in numpy, from the header's text: the rule from a frame's raw model index to a table entry, the
entry's device layout, the pack function and every refusal.  tests/test_model_plan.py and tests/test_models_sanitized.py
hold the compiled header against it; tests/model_cases.py has the cases both feed it."""
import numpy as np

MAX_MODELS, MAX_CLASSES, MAX_DF, NFEAT = 64, 8, 28, 1200

# one entry as the device holds it: weights [28][1200] f32, rho [28] f64, labels [8] i32, n_class i32, padding to a multiple of 16 bytes
ENTRY = np.dtype([("weights", "<f4", (MAX_DF, NFEAT)), ("rho", "<f8", (MAX_DF,)), ("labels", "<i4", (MAX_CLASSES,)), ("n_class", "<i4"), ("pad", "<i4", (3,))])
assert ENTRY.itemsize == 134672 and ENTRY.itemsize % 16 == 0
assert ENTRY.fields["rho"][1] == 134400 and ENTRY.fields["labels"][1] == 134624 and ENTRY.fields["n_class"][1] == 134656


def n_df(n_class):
    return n_class * (n_class - 1) // 2


def frame_model_eff(idx, n_models):
    """((uint32_t)idx < (uint32_t)n_models) ? idx : 0, for any int32 pair"""
    return idx if (idx & 0xFFFFFFFF) < (n_models & 0xFFFFFFFF) else 0


def model(weights, rho, labels, n_class=None):
    """a host rmcv_svm_model: any of the three arrays may be None (a null pointer); n_class defaults to len(labels)"""
    return {"weights": weights, "rho": rho, "labels": labels, "n_class": len(labels) if n_class is None else n_class}


def models_refusal(models, n_models):
    """the message rmcv_svm_load_models refuses the table with, or None; models None: a null table"""
    if n_models < 1 or n_models > MAX_MODELS:
        return "rmcv_svm_load_models: n_models %d is out of range (1 .. %d)" % (n_models, MAX_MODELS)
    if models is None:
        return "rmcv_svm_load_models: a null pointer"
    for m in range(n_models):
        M = models[m]
        if M["weights"] is None or M["rho"] is None or M["labels"] is None:
            return "rmcv_svm_load_models: model %d: a null pointer" % m
        if M["n_class"] < 2 or M["n_class"] > MAX_CLASSES:
            return "rmcv_svm_load_models: model %d: n_class %d is out of range (2 .. %d)" % (m, M["n_class"], MAX_CLASSES)
        d = n_df(M["n_class"])
        w = np.asarray(M["weights"], np.float32).reshape(-1)[:d * NFEAT]
        bad = np.flatnonzero(~np.isfinite(w))
        if len(bad):
            return "rmcv_svm_load_models: model %d: weight %d of decision function %d is not finite" % (m, bad[0] % NFEAT, bad[0] // NFEAT)
        bad = np.flatnonzero(~np.isfinite(np.asarray(M["rho"], np.float64).reshape(-1)[:d]))
        if len(bad):
            return "rmcv_svm_load_models: model %d: rho %d is not finite" % (m, bad[0])
    return None


def pack(models):
    """the table's bytes: entry after entry, decision functions and labels a model does not have zero-filled"""
    t = np.zeros(len(models), ENTRY)
    for k, M in enumerate(models):
        c, d = M["n_class"], n_df(M["n_class"])
        t[k]["weights"][:d] = np.asarray(M["weights"], np.float32).reshape(-1)[:d * NFEAT].reshape(d, NFEAT)
        t[k]["rho"][:d] = np.asarray(M["rho"], np.float64).reshape(-1)[:d]
        t[k]["labels"][:c] = np.asarray(M["labels"], np.int32).reshape(-1)[:c]
        t[k]["n_class"] = c
    return t.tobytes()


def frame_models_refusal(idx, n_models):
    """what the host setter refuses of its indices: the first frame whose index is not an entry"""
    for f, i in enumerate(idx):
        if frame_model_eff(int(i), n_models) != int(i):
            return "rmcv_batch_set_frame_models: frame %d: model %d is outside the table (0 .. %d)" % (f, int(i), n_models - 1)
    return None


def pipeline_models_refusal(n_frames, idx_frames, tables_agree):
    if n_frames == idx_frames:
        return None if tables_agree else ("n_models differs between the pipeline's contexts: load the same models into EVERY slot "
                                          "(rmcv_pipeline_context, rmcv_svm_load_models)")
    return "the batch has %d frames, the pipeline's model index table %d (rmcv_pipeline_set_frame_models)" % (n_frames, idx_frames)
