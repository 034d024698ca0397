"""The dataset harvest's novelty rule restated in numpy from the TEXT at the head of rmcv_amd/csrc/device_novelty.h -- not from
its code: whole-array distances where the header loops over bytes and ring rows.

    icon_sad(a, b) = sum |a[i] - b[i]| over 1200 bytes;
    per stream: pushed, and a ring [R][1200] in which the row pushed as number k lies at position k % R; it holds rows number
    max(0, pushed - R) .. pushed - 1;
    candidates in order; d = min icon_sad(row, r) over the rows the stream's ring holds at that moment (rows pushed earlier in the same
    append included); an empty ring gives no d and the candidate is kept; d <= T: near (not kept, near += 1); otherwise kept and pushed --
    whether or not the dataset has a slot for it; kept rows are numbered stream-major, kept row k goes to slot count + k, a slot >= capacity
    is dropped.  R == 0: every candidate is kept, no state."""
import numpy as np

ROW = 1200
SAD_MAX = 306000
RING_MAX = 8
SKIP = -2**31
NO_SAD = 2**31 - 1       # min_sad of a candidate that met an empty ring
NO_IDENTITY = -2**31


def sad(a, b):
    return int(np.abs(np.asarray(a, np.int64) - np.asarray(b, np.int64)).sum())


class State:
    """the novelty state of a dataset with `streams` rings of depth R"""

    def __init__(self, streams, R):
        self.R = int(R)
        self.rings = np.zeros((streams, self.R, ROW), np.uint8)
        self.pushed = np.zeros(streams, np.int64)
        self.near = 0

    def copy(self):
        s = State(len(self.pushed), self.R)
        s.rings, s.pushed, s.near = self.rings.copy(), self.pushed.copy(), self.near
        return s


def append(state, T, rows, n_rows, labels):
    """one append over rows [sum n_rows, 1200], stream-major -> (keep bool [sum n_rows], min_sad int64 [sum n_rows], the most rows a stream
    pushed in this call).  A skipped stream's rows are stepped over: keep False, min_sad NO_SAD.  Mutates `state`."""
    rows = np.asarray(rows, np.uint8).reshape(-1, ROW)
    keep, dist = np.zeros(len(rows), bool), np.full(len(rows), NO_SAD, np.int64)
    R, at, most = state.R, 0, 0
    for s, (n, label) in enumerate(zip(n_rows, labels)):
        first = state.pushed[s]
        for i in range(at, at + int(n)):
            if label == SKIP:
                continue
            if R == 0:
                keep[i] = True
                continue
            held = np.arange(max(0, state.pushed[s] - R), state.pushed[s]) % R          # the positions of the rows the ring holds
            if len(held):
                dist[i] = np.abs(state.rings[s, held].astype(np.int64) - rows[i].astype(np.int64)).sum(axis=1).min()
            if len(held) and dist[i] <= T:
                state.near += 1
                continue
            keep[i] = True
            state.rings[s, state.pushed[s] % R] = rows[i]
            state.pushed[s] += 1
        most = max(most, int(state.pushed[s] - first))
        at += int(n)
    return keep, dist, most


def place(keep, n_rows, labels, count, capacity, dropped, tag):
    """where the kept candidates go: -> (items int64 [m, 3] = (index into rows, slot) ..., metadata tuples, count', dropped').  items: (row
    index, slot) of every kept row that has a slot; meta: (tag, frame, armour, label, identity, win_x, win_y) per item"""
    stream = np.repeat(np.arange(len(n_rows)), n_rows)
    index = np.concatenate([np.arange(n) for n in n_rows]) if len(n_rows) else np.zeros(0, np.int64)
    kept = np.flatnonzero(keep)
    slot = count + np.arange(len(kept))
    fits = slot < capacity
    items = np.stack([kept[fits], slot[fits]], axis=1).reshape(-1, 2)
    meta = [(int(tag), int(stream[i]), int(index[i]), int(labels[stream[i]]), NO_IDENTITY, 0, 0) for i in kept[fits]]
    return items, meta, min(count + len(kept), capacity), dropped + max(0, count + len(kept) - capacity)
