"""The cases tests/test_model_plan.py and tests/test_models_sanitized.py feed tests/models_san_main.cpp (rmcv_amd/csrc/model_plan.h
compiled for the host), how they are written into its case file, and what it must answer according to tests/model_ref.py."""
import struct

import numpy as np

import model_ref as R

RULE_N = (1, 2, 64)


def rule_indices(n):
    return (-2**31, -1, 0, 1, n - 1, n, 2**31 - 1)


def rand_model(seed, n_class, labels=None):
    rng = np.random.default_rng(seed)
    d = R.n_df(n_class)
    w = (rng.standard_normal((d, R.NFEAT)) * 1e-3).astype(np.float32)
    rho = rng.standard_normal(d) * 0.05
    return R.model(w, rho, np.asarray(labels if labels is not None else rng.integers(-50, 50, n_class), np.int32))


def with_value(m, field, at, v):
    out = dict(m)
    a = np.array(m[field], copy=True)
    a.reshape(-1)[at] = v
    out[field] = a
    return out


def tables():
    """(name, models or None, n_models): the tables that pack (entries of 2, 3, 7 and 8 classes; 1 of 2; 64 of 8) and one for every refusal"""
    four = [rand_model(1, 2), rand_model(2, 3), rand_model(3, 7), rand_model(4, 8)]
    out = [("one of two classes", [rand_model(5, 2)], 1), ("2, 3, 7 and 8 classes", four, 4),
           ("64 of 8 classes", [rand_model(100 + k, 8) for k in range(64)], 64)]
    for n in (0, -1, 65):
        out.append(("n_models %d" % n, four, n))
    out.append(("a null table", None, 1))
    for field in ("weights", "rho", "labels"):
        bad = list(four)
        bad[1] = dict(four[1], **{field: None})
        out.append(("null " + field, bad, 4))
    for n_class in (1, 9, 0, -3):
        bad = list(four)
        bad[2] = dict(four[2], n_class=n_class)
        out.append(("n_class %d" % n_class, bad, 4))
    for v in (np.inf, -np.inf, np.nan):
        bad = list(four)
        bad[1] = with_value(four[1], "weights", 2 * R.NFEAT + 7, v)
        out.append(("weight %r" % v, bad, 4))
        bad = list(four)
        bad[3] = with_value(four[3], "rho", 27, v)
        out.append(("rho %r" % v, bad, 4))
    # the first refusal wins: entry 0's rho before entry 1's class count; a weight before a rho of the same entry
    bad = [with_value(four[0], "rho", 0, np.nan), dict(four[1], n_class=9)] + four[2:]
    out.append(("order across entries", bad, 4))
    bad = [with_value(with_value(four[0], "rho", 0, np.nan), "weights", R.NFEAT - 1, np.inf)] + four[1:]
    out.append(("order inside an entry", bad, 4))
    return out


def setter_cases():
    """(n_models, indices) for the host setter's refusal"""
    return [(4, [1, 2, 3, 0]), (4, [0, 4, -1]), (4, [3, 3, -1]), (1, [0, 0, 0, 1]), (64, [63, 0, 64]), (2, [2**31 - 1]), (2, [0, 1, -2**31])]


def encode():
    b = bytearray()
    ts = tables()
    b += struct.pack("<i", len(ts))
    for _, models, n in ts:
        given = [] if models is None else models[:max(0, min(n, len(models)))] if 1 <= n <= R.MAX_MODELS else []
        b += struct.pack("<iii", n, 1 if models is None else 0, len(given))
        for M in given:
            c = M["n_class"]
            d = R.n_df(c) if 2 <= c <= R.MAX_CLASSES else 0
            mask = (1 if M["weights"] is None else 0) | (2 if M["rho"] is None else 0) | (4 if M["labels"] is None else 0)
            b += struct.pack("<iii", c, mask, d)
            if d:
                w = np.zeros(d * R.NFEAT, np.float32) if M["weights"] is None else np.asarray(M["weights"], "<f4").reshape(-1)[:d * R.NFEAT]
                r = np.zeros(d) if M["rho"] is None else np.asarray(M["rho"], "<f8").reshape(-1)[:d]
                lab = np.zeros(c, np.int32) if M["labels"] is None else np.asarray(M["labels"], "<i4").reshape(-1)[:c]
                b += w.astype("<f4").tobytes() + r.astype("<f8").tobytes() + lab.astype("<i4").tobytes()
    ss = setter_cases()
    b += struct.pack("<i", len(ss))
    for n, idx in ss:
        b += struct.pack("<ii", n, len(idx)) + np.asarray(idx, "<i4").tobytes()
    return bytes(b)


def expected():
    """(the lines the program prints, the bytes it writes)"""
    lines, blob = [], b""
    for i, (_, models, n) in enumerate(tables()):
        no = R.models_refusal(models, n)
        if no:
            lines.append("T %d : %s" % (i, no))
        else:
            packed = R.pack(models[:n])
            lines.append("T %d : ok %d" % (i, len(packed)))
            blob += packed
    for n in RULE_N:
        for idx in rule_indices(n):
            lines.append("R %d %d : %d" % (n, idx, R.frame_model_eff(idx, n)))
    for i, (n, idx) in enumerate(setter_cases()):
        lines.append("F %d : %s" % (i, R.frame_models_refusal(idx, n) or "-"))
    for nf in (4, 5):
        for tf in (4, 5):
            for agree in (0, 1):
                lines.append("P %d %d %d : %s" % (nf, tf, agree, R.pipeline_models_refusal(nf, tf, bool(agree)) or "-"))
    lines.append("S 8128 0")   # run_steps: 127 stage masks x 64 settings compared, none off the rule
    return lines, blob
