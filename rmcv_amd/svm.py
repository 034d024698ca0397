"""Training the icon classifier: the reference's executable/svm/optimizer.cpp on arrays.

    data = Dataset(["1", "2", "3", "4", "5", "Sentry", "Negtive"])
    data.add(0, icons_of_class_0)                      # uint8 [m, 1200] rows as Context.icons / classify_armours hand them out
    train, held_out = data.sample(0.6, seed=1)         # rm::svm::dataset::sample, seeded instead of the wall clock
    model = train_auto(*train.format_data(), ctx=ctx)  # cv::ml::SVM::trainAuto's role: rmcv_svm_train (ctx) / rmcv_svm_train_host (ctx=None)
    model.load_into(ctx)                               # rmcv_svm_load: RMCV_STAGE_IDENTITY and Context.svm_predict use it

No image files are read here and no XML is written: Model.save / Model.load keep the model in a small container of the library's own.
"""
import ctypes as C
import struct

import numpy as np

from . import abi
from .abi import RmcvError, SvmTrainParams, SvmTrainReport, lib, ptr

PHASES = ("gram", "search_smo", "search_weights", "search_predict", "final_smo", "final_weights")  # rmcv_svm_train_report::phase_ms
MODEL_MAGIC = b"RMCVSVM1"  # then <i n_class, int32 labels[n_class], float64 rho[n_df], float32 weights[n_df][1200], little endian


def _rows(samples):
    s = np.ascontiguousarray(samples, np.uint8)
    s = s.reshape(len(s), -1) if s.size else s.reshape(0, abi.SVM_FEATURES)
    if s.shape[1] != abi.SVM_FEATURES:
        raise RmcvError(abi.ERR_BAD_ARG, "rows must have %d bytes (20 x 20 x BGR)" % abi.SVM_FEATURES)
    return s


def default_train_params(**kw):
    """rmcv_svm_train_defaults, then the keywords: eps, max_iter, k_fold, c_grid (a sequence: n_c is its length)"""
    p = SvmTrainParams()
    lib().rmcv_svm_train_defaults(C.byref(p))
    for k, v in kw.items():
        if k == "c_grid":
            v = [float(c) for c in v]
            if not 1 <= len(v) <= abi.SVM_MAX_GRID:
                raise RmcvError(abi.ERR_BAD_ARG, "c_grid holds 1 .. %d values" % abi.SVM_MAX_GRID)
            p.n_c = len(v)
            for i in range(abi.SVM_MAX_GRID):
                p.c_grid[i] = v[i] if i < len(v) else 0.0
        elif k in ("eps", "max_iter", "k_fold"):
            setattr(p, k, v)
        else:
            raise TypeError("unknown training parameter %r" % k)
    return p


class Dataset(dict):
    """rm::svm::dataset on arrays: class index -> uint8 [m, 1200]; `labels` names the indices (include/svm.h)"""

    def __init__(self, labels):
        super().__init__()
        self.labels = list(labels)

    def add(self, index, rows):
        rows = _rows(rows)
        self[int(index)] = np.concatenate([self[int(index)], rows]) if int(index) in self else rows
        return self

    def sample(self, ratio, seed):
        """src/svm.cpp:22-34: every class shuffled, its first int(float32(m) * float32(ratio)) rows to the head, the rest to the tail;
        the shuffle of class `index` is numpy's RandomState(seed + index).permutation, not the wall clock's"""
        head, tail = Dataset(self.labels), Dataset(self.labels)
        for index in sorted(self):
            rows = self[index][np.random.RandomState(int(seed) + index).permutation(len(self[index]))]
            split = int(np.float32(len(rows)) * np.float32(ratio))
            head[index], tail[index] = rows[:split], rows[split:]
        return head, tail

    def format_data(self):
        """src/svm.cpp:36-49 -> (samples uint8 [n, 1200], responses int32 [n]), classes in index order"""
        keys = sorted(self)
        if not keys:
            return np.zeros((0, abi.SVM_FEATURES), np.uint8), np.zeros(0, np.int32)
        return np.concatenate([self[k] for k in keys]), np.concatenate([np.full(len(self[k]), k, np.int32) for k in keys])


class Model:
    """a linear one-vs-one C-SVC as rmcv_svm_load takes it, with what training reported"""

    def __init__(self, weights, rho, labels, report=None):
        self.labels = np.ascontiguousarray(labels, np.int32)
        n_df = len(self.labels) * (len(self.labels) - 1) // 2
        self.weights = np.ascontiguousarray(weights, np.float32).reshape(n_df, abi.SVM_FEATURES)
        self.rho = np.ascontiguousarray(rho, np.float64).reshape(n_df)
        self.report = report or {}

    def load_into(self, ctx):
        ctx.svm_load(self.weights, self.rho, self.labels)
        return ctx

    def as_entry(self):
        """(weights, rho, labels): one entry of Context.svm_load_models' table"""
        return self.weights, self.rho, self.labels

    def predict(self, samples):
        """rmcv_svm_predict_host: the labels of uint8 [n, 1200] rows, on the CPU"""
        s = _rows(samples)
        out = np.zeros(len(s), np.int32)
        rc = lib().rmcv_svm_predict_host(ptr(self.weights), ptr(self.rho), ptr(self.labels), len(self.labels), ptr(s) if len(s) else None, len(s),
                                         ptr(out) if len(s) else None)
        if rc:
            raise RmcvError(rc, "rmcv_svm_predict_host")
        return out

    def save(self, path):
        with open(path, "wb") as f:
            f.write(MODEL_MAGIC + struct.pack("<i", len(self.labels)) + self.labels.astype("<i4").tobytes() + self.rho.astype("<f8").tobytes() +
                    self.weights.astype("<f4").tobytes())

    @classmethod
    def load(cls, path):
        b = open(path, "rb").read()
        if len(b) < 12 or b[:8] != MODEL_MAGIC:
            raise RmcvError(abi.ERR_BAD_ARG, "%s is no rmcv svm model" % path)
        (n_class,) = struct.unpack("<i", b[8:12])
        n_df = n_class * (n_class - 1) // 2
        if not 2 <= n_class <= 8 or len(b) != 12 + 4 * n_class + 8 * n_df + 4 * n_df * abi.SVM_FEATURES:
            raise RmcvError(abi.ERR_BAD_ARG, "%s: the sizes of the model do not agree with the file's" % path)
        at = 12
        labels = np.frombuffer(b, "<i4", n_class, at)
        rho = np.frombuffer(b, "<f8", n_df, at + 4 * n_class)
        weights = np.frombuffer(b, "<f4", n_df * abi.SVM_FEATURES, at + 4 * n_class + 8 * n_df)
        return cls(weights, rho, labels)


def load_models(ctx, models):
    """rmcv_svm_load_models: the Models `models` as ctx's model table, one per colour or per robot (Context.set_frame_models picks per frame)"""
    ctx.svm_load_models([m.as_entry() for m in models])
    return ctx


def gram(samples, ctx=None):
    """the exact int32 Gram matrix of uint8 [n, 1200] rows: rmcv_svm_gram on ctx's device, rmcv_svm_gram_host without one"""
    s = _rows(samples)
    out = np.zeros((len(s), len(s)), np.int32)
    if ctx is None:
        rc = lib().rmcv_svm_gram_host(ptr(s), len(s), ptr(out))
        if rc:
            raise RmcvError(rc, "rmcv_svm_gram_host: 1 .. %d rows" % abi.SVM_MAX_SAMPLES)
    else:
        ctx._chk(lib().rmcv_svm_gram(ctx._h, ptr(s), len(s), ptr(out)))
    return out


def train_auto(samples, responses, perm=None, ctx=None, alphas=False, **params):
    """cv::ml::SVM::trainAuto's role under the library's own rule -> Model.  samples uint8 [n, 1200], responses int [n], perm a permutation
    of the rows (None: identity) from which the folds are cut; params: default_train_params' keywords.  ctx: the Context whose GPU trains
    (rmcv_svm_train); None: the sequential form on the CPU (rmcv_svm_train_host) -- the two agree bit for bit.  alphas: keep the returned
    model's alphas [n_df, n] in report["alpha"]."""
    s = _rows(samples)
    r = np.ascontiguousarray(responses, np.int32).reshape(-1)
    if len(r) != len(s):
        raise RmcvError(abi.ERR_BAD_ARG, "one response per row")
    q = None if perm is None else np.ascontiguousarray(perm, np.int32).reshape(-1)
    if q is not None and len(q) != len(s):
        raise RmcvError(abi.ERR_BAD_ARG, "perm has one entry per row")
    p = default_train_params(**params)
    weights, rho, labels = np.zeros((abi.SVM_MAX_DF, abi.SVM_FEATURES), np.float32), np.zeros(abi.SVM_MAX_DF), np.zeros(8, np.int32)
    n_class, rep = C.c_int32(0), SvmTrainReport()
    alpha = np.zeros((abi.SVM_MAX_DF, max(len(s), 1))) if alphas else None
    rep.alpha_out = None if alpha is None else alpha.ctypes.data
    args = [ptr(s) if len(s) else None, ptr(r) if len(r) else None, len(s), ptr(q), C.byref(p), ptr(weights), ptr(rho), ptr(labels), C.byref(n_class), C.byref(rep)]
    rc = lib().rmcv_svm_train_host(*args) if ctx is None else lib().rmcv_svm_train(ctx._h, *args)
    if rc:
        raise RmcvError(rc, rep.message.decode() or (lib().rmcv_last_error(ctx._h).decode() if ctx is not None else "rmcv_svm_train_host"))
    n_df = rep.n_df
    report = {"best_c": rep.best_c, "best_index": rep.best_index, "cv_errors": [int(v) for v in rep.cv_errors[:p.n_c]], "iterations": np.array(rep.iterations[:n_df]),
              "converged": np.array(rep.converged[:n_df]), "objective": np.array(rep.objective[:n_df]), "phase_ms": dict(zip(PHASES, rep.phase_ms))}
    if alpha is not None:
        report["alpha"] = alpha[:n_df].copy()
    return Model(weights[:n_df], rho[:n_df], labels[:n_class.value], report)
