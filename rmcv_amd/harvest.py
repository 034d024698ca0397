"""Dataset harvest: the reference's executable/svm/labeler.cpp on the device.

    ds = DeviceDataset(ctx, 4096)
    ctx.upload(frames); ctx.run(params, STAGE_ALL)       # no model needed
    ctx.harvest(ds, labels)                              # one label per frame (= per stream of a labelling session); HARVEST_SKIP: none
    pipeline.set_harvest(ds, labels)                     # ... or every following submit appends, tag = its ticket
    train, held_out = ds.sample(0.6, seed=1)             # per-label index lists, rm::svm::dataset::sample's rule, seeded
    model = ds.train_auto(np.concatenate(list(train.values())))   # rmcv_svm_train_dataset: the rows never leave the device
    model.load_into(ctx); ds.predict(rows)               # rmcv_svm_predict_dataset
Novelty: a dataset that skips near-duplicates of the icons it kept last from the same stream.
    ds.set_novelty(8, 2000)                              # per stream, remember the last 8 kept rows; a candidate within SAD 2000 of one is not kept
    ds.novelty                                           # {"ring_rows": 8, "max_sad": 2000, "near": candidates skipped so far}
    ds.append_rows(rows, n_rows, labels)                 # rows the caller already has go through the same rule
"""
import ctypes as C

import numpy as np

from . import abi, svm
from .abi import HARVEST_META, RmcvError, SvmTrainReport, lib, ptr


def harvest_plan(n_armours, status, labels, identity=None, max_armours=None, flags=0, count=0, capacity=1, dropped=0):
    """the rule on the host (rmcv_harvest_plan_host: device_harvest.h compiled for the host) -> (items [(frame, armour, slot)] as an int32
    [n, 3] array, count, dropped).  identity: [n_frames, max_armours] (needed with HARVEST_MISSES)."""
    n = np.ascontiguousarray(n_armours, np.int32).reshape(-1)
    st = np.ascontiguousarray(status, np.int32).reshape(-1)
    lb = np.ascontiguousarray(labels, np.int32).reshape(-1)
    if not len(n) == len(st) == len(lb):
        raise RmcvError(abi.ERR_BAD_ARG, "one count, status word and label per frame")
    ident = None
    if identity is not None:
        ident = np.ascontiguousarray(identity, np.int32).reshape(len(n), -1)
        max_armours = ident.shape[1] if max_armours is None else max_armours
        if ident.shape[1] != max_armours:
            raise RmcvError(abi.ERR_BAD_ARG, "identity is [n_frames, max_armours]")
    if max_armours is None:
        raise RmcvError(abi.ERR_BAD_ARG, "max_armours (or an identity table) is needed")
    cap = max(int(capacity) - int(count), 0)
    items = np.zeros((max(cap, 1), 3), np.int32)
    n_items, now, drop = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    rc = lib().rmcv_harvest_plan_host(ptr(n) if len(n) else None, ptr(st) if len(n) else None, ptr(lb) if len(n) else None, ptr(ident), len(n), int(max_armours),
                                      int(flags), int(count), int(capacity), int(dropped), ptr(items), cap, C.byref(n_items), C.byref(now), C.byref(drop))
    if rc:
        raise RmcvError(rc, "rmcv_harvest_plan_host")
    return items[:n_items.value].copy(), now.value, drop.value


def icon_sad(a, b):
    """rmcv_icon_sad: the sum of absolute byte differences of two icon rows (uint8 [1200]), 0 .. ICON_SAD_MAX"""
    a, b = np.ascontiguousarray(a, np.uint8).reshape(-1), np.ascontiguousarray(b, np.uint8).reshape(-1)
    if len(a) != abi.SVM_FEATURES or len(b) != abi.SVM_FEATURES:
        raise RmcvError(abi.ERR_BAD_ARG, "icon_sad: a row is 1200 bytes")
    return int(lib().rmcv_icon_sad(ptr(a), ptr(b)))


def _row_tables(rows, n_rows, labels):
    n = np.ascontiguousarray(n_rows, np.int32).reshape(-1)
    lb = np.ascontiguousarray(labels, np.int32).reshape(-1)
    r = np.ascontiguousarray(rows, np.uint8).reshape(-1, abi.SVM_FEATURES)
    if len(n) != len(lb) or (n < 0).any() or int(n.sum()) != len(r):
        raise RmcvError(abi.ERR_BAD_ARG, "rows is [sum(n_rows), 1200], stream-major, with one count (>= 0) and one label per stream")
    return r, n, lb


def harvest_novel(rows, n_rows, labels, ring_rows, max_sad, rings=None, pushed=None):
    """the novelty rule on the host (rmcv_harvest_novel_host: device_novelty.h compiled for the host) over rows laid out as for
    DeviceDataset.append_rows -> (keep uint8 [sum n_rows], min_sad int32 [sum n_rows] (INT32_MAX: no distance), near, rings, pushed).
    rings uint8 [n_streams, ring_rows, 1200] and pushed int64 [n_streams] are the state before the call (None: empty); the returned ones
    are copies behind it."""
    r, n, lb = _row_tables(rows, n_rows, labels)
    R = int(ring_rows)
    rg = np.zeros((len(n), max(R, 0), abi.SVM_FEATURES), np.uint8) if rings is None else np.array(rings, np.uint8).reshape(len(n), max(R, 0), abi.SVM_FEATURES)
    pu = np.zeros(len(n), np.int64) if pushed is None else np.array(pushed, np.int64).reshape(len(n))
    keep, sad, near = np.zeros(max(len(r), 1), np.uint8), np.zeros(max(len(r), 1), np.int32), C.c_int64(0)
    rc = lib().rmcv_harvest_novel_host(ptr(r) if len(r) else None, ptr(n) if len(n) else None, ptr(lb) if len(n) else None, len(n), R, int(max_sad),
                                       ptr(rg) if rg.size else None, ptr(pu) if len(n) else None, ptr(keep), ptr(sad), C.byref(near))
    if rc:
        raise RmcvError(rc, "rmcv_harvest_novel_host")
    return keep[:len(r)], sad[:len(r)], near.value, rg, pu


class DeviceDataset:
    """rmcv_dataset: `capacity` icon rows (uint8 [1200]) and their metadata in the memory of ctx's device"""

    def __init__(self, ctx, capacity):
        self._ctx = ctx
        h = C.c_void_p()
        ctx._chk(lib().rmcv_dataset_create(ctx._h, int(capacity), C.byref(h)))
        self._h, self.capacity = h, int(capacity)

    def close(self):
        if getattr(self, "_h", None):
            lib().rmcv_dataset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise RmcvError(rc, lib().rmcv_dataset_last_error(self._h).decode())

    def _counts(self):
        rows, dropped = C.c_int32(0), C.c_int64(0)
        self._chk(lib().rmcv_dataset_count(self._h, C.byref(rows), C.byref(dropped)))
        return rows.value, dropped.value

    @property
    def count(self):
        """rows held (waits for the last append)"""
        return self._counts()[0]

    @property
    def dropped(self):
        """rows that found the dataset full since the last clear()"""
        return self._counts()[1]

    def clear(self):
        self._chk(lib().rmcv_dataset_clear(self._h))

    def set_novelty(self, ring_rows, max_sad):
        """rmcv_dataset_set_novelty: from the next append on, per stream (= frame index of an append) the last `ring_rows` kept rows are
        remembered (0 .. HARVEST_RING_MAX; 0: off) and a candidate whose icon_sad to one of them is <= max_sad is not kept.  Waits for the
        last append; empties every ring."""
        self._chk(lib().rmcv_dataset_set_novelty(self._h, int(ring_rows), int(max_sad)))

    @property
    def novelty(self):
        """{"ring_rows", "max_sad", "near"}: the setting and the candidates skipped as near since the last clear() (waits for the last append)"""
        r, t, near = C.c_int(0), C.c_int32(0), C.c_int64(0)
        self._chk(lib().rmcv_dataset_novelty(self._h, C.byref(r), C.byref(t), C.byref(near)))
        return {"ring_rows": r.value, "max_sad": t.value, "near": near.value}

    def rings(self, first=0, n=None):
        """(rows uint8 [n, ring_rows, 1200], pushed int64 [n]) of streams first .. first + n - 1 (n None: to the last) as they lie: the row
        pushed as number k of a stream at position k % ring_rows, positions not yet written zero"""
        first = int(first)
        n = self._ctx.limits.max_frames - first if n is None else int(n)
        R = self.novelty["ring_rows"]
        rows, pushed = np.zeros((max(n, 0), R, abi.SVM_FEATURES), np.uint8), np.zeros(max(n, 0), np.int64)
        self._chk(lib().rmcv_dataset_get_rings(self._h, first, n, ptr(rows) if rows.size else None, ptr(pushed) if n > 0 else None))
        return rows, pushed

    def append_rows(self, rows, n_rows, labels, tag=0):
        """rmcv_dataset_append_rows: rows the caller already has (uint8 [sum(n_rows), 1200], stream-major: stream s gives n_rows[s]
        candidates in order, none under HARVEST_SKIP) through the rule of any other append, novelty included.  frame = the stream, armour =
        the index within it.  Asynchronous: count waits."""
        r, n, lb = _row_tables(rows, n_rows, labels)
        if len(r) == 0:
            r = np.zeros((1, abi.SVM_FEATURES), np.uint8)   # (a table to point at: no row of it is read)
        self._chk(lib().rmcv_dataset_append_rows(self._h, ptr(r), ptr(n) if len(n) else None, ptr(lb) if len(n) else None, len(n), int(tag)))

    def _range(self, first, n):
        first = int(first)
        return first, (self.count - first if n is None else int(n))

    def rows(self, first=0, n=None):
        """uint8 [n, 1200]: rows first .. first + n - 1 (n None: to the end)"""
        first, n = self._range(first, n)
        out = np.zeros((max(n, 0), abi.SVM_FEATURES), np.uint8)
        self._chk(lib().rmcv_dataset_get(self._h, first, n, ptr(out) if n > 0 else None, None))
        return out

    def meta(self, first=0, n=None):
        """the rows' metadata as a HARVEST_META record array"""
        first, n = self._range(first, n)
        out = np.zeros(max(n, 0), HARVEST_META)
        self._chk(lib().rmcv_dataset_get(self._h, first, n, None, ptr(out) if n > 0 else None))
        return out

    def device(self):
        """(d_rows, d_meta, d_count): device addresses of the rows, the metadata and the int32 count (rmcv_dataset_device: zero-copy)"""
        r, m, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._chk(lib().rmcv_dataset_device(self._h, C.byref(r), C.byref(m), C.byref(c)))
        return r.value, m.value, c.value

    def sample(self, ratio, seed):
        """rm::svm::dataset::sample on slot indices, seeded as svm.Dataset.sample is: per label (ascending), the slots of that label in
        order, shuffled by RandomState(seed + label).permutation; the first int(float32(m) * float32(ratio)) to the head, the rest to the
        tail -> (head, tail), each {label: int32 slots}"""
        labels = self.meta()["label"]
        head, tail = {}, {}
        for label in sorted(set(int(v) for v in labels)):
            slots = np.flatnonzero(labels == label).astype(np.int32)
            slots = slots[np.random.RandomState(int(seed) + label).permutation(len(slots))]
            split = int(np.float32(len(slots)) * np.float32(ratio))
            head[label], tail[label] = slots[:split], slots[split:]
        return head, tail

    def _index(self, rows):
        if rows is None:
            return None, self.count
        r = np.ascontiguousarray(rows, np.int32).reshape(-1)
        return r, len(r)

    def train_auto(self, rows=None, perm=None, ctx=None, **params):
        """rmcv_svm_train_dataset -> svm.Model: svm.train_auto on the rows `rows` (slot indices; None: every row) with their labels as
        responses, read where they lie.  Bit-identical to svm.train_auto(ds.rows()[rows], ds.meta()["label"][rows], perm, ctx=ctx)."""
        ctx = ctx or self._ctx
        r, n = self._index(rows)
        q = None if perm is None else np.ascontiguousarray(perm, np.int32).reshape(-1)
        if q is not None and len(q) != n:
            raise RmcvError(abi.ERR_BAD_ARG, "perm has one entry per row")
        p = svm.default_train_params(**params)
        weights, rho, labels = np.zeros((abi.SVM_MAX_DF, abi.SVM_FEATURES), np.float32), np.zeros(abi.SVM_MAX_DF), np.zeros(8, np.int32)
        n_class, rep = C.c_int32(0), SvmTrainReport()
        rep.alpha_out = None
        rc = lib().rmcv_svm_train_dataset(ctx._h, self._h, ptr(r), n, ptr(q), C.byref(p), ptr(weights), ptr(rho), ptr(labels), C.byref(n_class), C.byref(rep))
        if rc:
            raise RmcvError(rc, rep.message.decode() or lib().rmcv_last_error(ctx._h).decode())
        n_df = rep.n_df
        report = {"best_c": rep.best_c, "best_index": rep.best_index, "cv_errors": [int(v) for v in rep.cv_errors[:p.n_c]], "iterations": np.array(rep.iterations[:n_df]),
                  "converged": np.array(rep.converged[:n_df]), "objective": np.array(rep.objective[:n_df]), "phase_ms": dict(zip(svm.PHASES, rep.phase_ms))}
        return svm.Model(weights[:n_df], rho[:n_df], labels[:n_class.value], report)

    def predict(self, rows=None, ctx=None):
        """rmcv_svm_predict_dataset: the labels ctx's loaded model gives the rows `rows` (slot indices; None: every row), read in place"""
        ctx = ctx or self._ctx
        r, n = self._index(rows)
        out = np.zeros(n, np.int32)
        ctx._chk(lib().rmcv_svm_predict_dataset(ctx._h, self._h, ptr(r), n, ptr(out) if n else None))
        return out
