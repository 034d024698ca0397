"""Seeded calls for the novelty rule, shared by tests/test_novelty_cpu.py (rmcv_harvest_novel_host), tests/test_novelty_sanitized.py
(tests/novelty_san_main.cpp) and tests/test_gpu_novelty.py (DeviceDataset.append_rows): the smallest shapes at which k_harvest_novel can go
wrong.  A case is a dataset (ring depth R, threshold T, capacity, the creating context's max_frames `cap`) and the appends it sees in order;
expected(case) is what tests/novelty_ref.py makes of it, computed once.  census() asserts that the cases are what they claim."""
import collections
import functools

import numpy as np

import novelty_ref as R

Case = collections.namedtuple("Case", "name cap R T capacity appends")   # appends: [(rows u8 [sum n, 1200], n_rows, labels, tag)]
ROOMY = 1 << 20


def base_row(seed):
    return np.random.RandomState(seed).randint(1, 255, R.ROW).astype(np.uint8)   # (1 .. 254: a byte can move either way)


def bump(row, at, by=1):
    out = row.copy()
    out[at] += by
    return out


def tail_diff(row, total):
    """`row` with differences only in bytes 1024 .. 1199 (the words past a first 64-lane sweep of four), summing to exactly `total`"""
    out, left = row.astype(np.int64), total
    for i in range(1024, R.ROW):
        step = min(left, 255 - out[i]) if out[i] < 128 else -min(left, out[i])
        out[i] += step
        left -= abs(step)
    assert left == 0 and R.sad(out, row) == total and (out[:1024] == row[:1024]).all()
    return out.astype(np.uint8)


def one(rows, n_rows, labels, tag=0):
    rows = np.ascontiguousarray(np.asarray(rows, np.uint8).reshape(-1, R.ROW))
    assert len(rows) == sum(n_rows) and len(n_rows) == len(labels)
    rows.setflags(write=False)
    return rows, np.asarray(n_rows, np.int32), np.asarray(labels, np.int32), tag


def seeded(n_streams, depth, seed):
    """per stream a count from 0, 1, R, R + 1, 2 R + 1, 65 (in turn, starting at a seeded place) of rows drawn from three far-apart rows of
    the stream's, each with up to six bytes moved by one: against T = 3 some are near the row they came from and some are not"""
    r = np.random.RandomState(seed)
    counts = [0, 1, depth, depth + 1, 2 * depth + 1, 65]
    n_rows = [counts[(s + seed) % 6] for s in range(n_streams)]
    rows = []
    for s in range(n_streams):
        pool = r.randint(1, 255, (3, R.ROW)).astype(np.uint8)
        for _ in range(n_rows[s]):
            row = pool[r.randint(3)].copy()
            at = r.choice(R.ROW, r.randint(0, 7), replace=False)
            row[at] += 1
            rows.append(row)
    return one(rows, n_rows, [s % 7 for s in range(n_streams)], seed)


@functools.lru_cache(maxsize=None)
def cases():
    b = base_row(1)
    zeros, full = np.zeros(R.ROW, np.uint8), np.full(R.ROW, 255, np.uint8)
    a_, b_ = base_row(2), base_row(3)
    out = []
    # (a) a copy, (b) one byte off by one at 0, 1023, 1024, 1199
    singles = [b, b.copy(), bump(b, 0), bump(b, 1023), bump(b, 1024), bump(b, 1199)]
    for T in (0, 1):
        out.append(Case("copy_and_off_by_one_T%d" % T, 8, 2, T, ROOMY, [one(singles, [6], [5])]))
    # (c) differences only in bytes 1024 .. 1199 summing to exactly T and to T + 1: two streams, one decision each way
    T = 5000
    out.append(Case("tail_words_T_and_T_plus_1", 8, 1, T, ROOMY, [one([b, tail_diff(b, T), b, tail_diff(b, T + 1)], [2, 2], [1, 2])]))
    # (d) all 0 against all 255: 306000
    for T in (R.SAD_MAX - 1, R.SAD_MAX):
        out.append(Case("extremes_T%d" % T, 8, 1, T, ROOMY, [one([zeros, full], [2], [0])]))
    # (e) A, B, A: depth 1 forgets, depth 2 remembers
    for depth in (1, 2):
        out.append(Case("aba_R%d" % depth, 8, depth, 0, ROOMY, [one([a_, b_, a_], [3], [4])]))
    # stream counts 1, 3, 4, 5, 8 (4 and 5 straddle a workgroup's four wavefronts) and 264 (the plan's two frames per thread) x ring depths;
    # two appends each: the second meets the rings the first left, and skips a stream that has rows to give
    for n_streams, depth, cap in ((1, 8, 8), (3, 1, 8), (4, 2, 8), (5, 8, 8), (8, 2, 8), (8, 1, 8), (264, 2, 264), (264, 8, 264)):
        first, second = seeded(n_streams, depth, 10 + n_streams), seeded(n_streams, depth, 11 + n_streams)
        labels = second[2].copy()
        skip = next((s for s in range(n_streams) if second[1][s] > 0 and first[1][s] > 0), None)
        if skip is not None:
            labels[skip] = R.SKIP
        out.append(Case("seeded_%d_streams_R%d" % (n_streams, depth), cap, depth, 3, ROOMY, [first, (second[0], second[1], labels, second[3])]))
    # a capacity that cuts inside a stream's kept rows: rings, pushed and near are those of the unbounded run
    roomy = Case("capacity_unbounded", 8, 2, 3, ROOMY, [seeded(5, 2, 40), seeded(5, 2, 41)])
    e = _run(roomy)
    n2 = roomy.appends[1][1]
    per_stream = np.array([e["keeps"][1][o:o + n].sum() for o, n in zip(np.cumsum(np.r_[0, n2[:-1]]), n2)], np.int64)   # kept rows per stream of the second append
    s = int(np.argmax(per_stream >= 2))
    assert per_stream[s] >= 2
    cut = e["counts"][0] + int(per_stream[:s].sum()) + 1                                                      # one row of stream s fits, the next does not
    out += [roomy, Case("capacity_cuts_a_stream", 8, 2, 3, cut, roomy.appends)]
    # novelty off: the rule of device_harvest.h alone
    out.append(Case("ring_rows_0", 8, 0, 0, ROOMY, [seeded(4, 2, 50)]))
    return tuple(out)


def _run(case):
    state = R.State(case.cap, case.R)
    count = dropped = 0
    rows, meta, keeps, sads, mosts, counts, states = [], [], [], [], [], [], []
    for r, n, lb, tag in case.appends:
        keep, dist, most = R.append(state, case.T, r, n, lb)
        items, m, count, dropped = R.place(keep, n, lb, count, case.capacity, dropped, tag)
        rows += [r[i] for i, _ in items]
        meta += m
        keeps.append(keep), sads.append(dist), mosts.append(most), counts.append(count), states.append(state.copy())
    return {"rows": np.array(rows, np.uint8).reshape(len(rows), R.ROW), "meta": meta, "count": count, "dropped": dropped, "near": state.near,
            "rings": state.rings, "pushed": state.pushed, "keeps": keeps, "sads": sads, "mosts": mosts, "counts": counts, "states": states}


_expected = {}


def expected(case):
    """what tests/novelty_ref.py makes of the case (computed once, shared; leave it unchanged)"""
    if case.name not in _expected:
        _expected[case.name] = _run(case)
    return _expected[case.name]


def census():
    """the cases are what they claim: kept and near candidates, an equality d == T, a ring that wraps inside one append, an empty ring, a
    dropped row, a skipped stream with an untouched ring, every stream count, candidate count and depth the kernel's paths differ at"""
    seen = collections.Counter()
    streams, counts, depths = set(), set(), set()
    for c in cases():
        e = expected(c)
        depths.add(c.R)
        before = R.State(c.cap, c.R)
        for (r, n, lb, _), keep, dist, most, after in zip(c.appends, e["keeps"], e["sads"], e["mosts"], e["states"]):
            streams.add(len(n))
            counts.update((int(v), int(v) - c.R, int(v) - 2 * c.R) for v in n)
            live = np.repeat(lb != R.SKIP, n)
            seen["kept"] += int(keep.sum())
            seen["near"] += int((live & ~keep).sum())
            seen["equal"] += int((live & (dist == c.T)).sum()) if c.R else 0
            seen["empty"] += int((live & (dist == R.NO_SAD)).sum()) if c.R else 0
            seen["wrap"] += most > c.R > 0
            for s in np.flatnonzero((lb == R.SKIP) & (n > 0)):
                assert np.array_equal(after.rings[s], before.rings[s]) and after.pushed[s] == before.pushed[s]
                seen["skipped_with_a_ring"] += int(before.pushed[s] > 0)
            before = after
        seen["dropped"] += e["dropped"]
        assert e["count"] <= c.capacity
    assert all(seen[k] > 0 for k in ("kept", "near", "equal", "empty", "wrap", "dropped", "skipped_with_a_ring")), seen
    assert {1, 3, 4, 5, 8, 264} <= streams and {0, 1, 2, 8} <= depths
    assert {(0, 0 - d, 0 - 2 * d) for d in (1, 2, 8)} <= counts                                      # no candidates
    assert all((d, 0, -d) in counts and (d + 1, 1, 1 - d) in counts and (2 * d + 1, d + 1, 1) in counts and (65, 65 - d, 65 - 2 * d) in counts
               for d in (1, 2, 8)), counts                                                           # R, R + 1, 2 R + 1 and 65 at every depth
    cut, roomy = (next(c for c in cases() if c.name == k) for k in ("capacity_cuts_a_stream", "capacity_unbounded"))
    a, b = expected(cut), expected(roomy)
    assert a["dropped"] > 0 and a["near"] == b["near"] and np.array_equal(a["rings"], b["rings"]) and np.array_equal(a["pushed"], b["pushed"])
    assert np.array_equal(a["rows"], b["rows"][:a["count"]]) and a["count"] < b["count"]             # a prefix of the unbounded dataset
    assert a["meta"][-1][1] == b["meta"][a["count"]][1]                                               # ... cut inside one stream's kept rows
    return seen
