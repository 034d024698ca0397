"""The dataset harvest's rule restated in numpy from the TEXT at the head of rmcv_amd/csrc/device_harvest.h -- not from its
code: whole-array operations where the header loops and scans.

    frame f contributes nothing when label[f] == SKIP or status[f] carries an RMCV_FRAME_OVF_* bit;
    otherwise its candidates are armours 0 .. min(n[f], max_armours) - 1 in table order;
    MISSES keeps a candidate only when identity != label[f]; without it every candidate is kept;
    kept rows are numbered frame-major, then armour-major; kept row k goes to slot count + k;
    a row whose slot is >= capacity is dropped; count' = min(count + kept, capacity); dropped' = dropped + max(0, count + kept - capacity).
"""
import numpy as np

SKIP = -2**31
MISSES = 1
OVF = 1 | 2 | 4 | 8   # RMCV_FRAME_OVF_CONTOURS | _POINTS | _BLOBS | _ARMOURS
NO_IDENTITY = -2**31  # rmcv_harvest_meta::identity of a run without an identity stage


def plan(n_armours, status, labels, identity, max_armours, flags, count, capacity, dropped=0):
    """-> (items int32 [m, 3] = (frame, armour, slot) of every row that gets a slot, count', dropped')"""
    n = np.asarray(n_armours, np.int64).reshape(-1)
    status = np.asarray(status, np.int64).reshape(-1)
    labels = np.asarray(labels, np.int64).reshape(-1)
    live = (labels != SKIP) & ((status & OVF) == 0)
    cand = np.where(live, np.clip(n, 0, max_armours), 0)
    keep = np.arange(max_armours)[None, :] < cand[:, None]                # [frame, armour]
    if flags & MISSES:
        keep &= np.asarray(identity, np.int64).reshape(len(n), max_armours) != labels[:, None]
    frame, armour = np.nonzero(keep)                                      # row-major: frame-major, then armour-major
    slot = count + np.arange(len(frame))
    fits = slot < capacity
    items = np.stack([frame[fits], armour[fits], slot[fits]], axis=1).astype(np.int32).reshape(-1, 3)
    kept = len(frame)
    return items, min(count + kept, capacity), dropped + max(0, count + kept - capacity)


def expected_meta(items, labels, identity, tag, origins=None):
    """what rmcv_harvest_meta holds of `items` apart from the icon quadrilateral: (tag, frame, armour, label, identity, win_x, win_y) per row.
    identity: [frame, max_armours] or None (no identity stage); origins: the effective window origins [frame, 2] or None"""
    out = []
    for f, a, _ in items:
        ident = NO_IDENTITY if identity is None else int(identity[f][a])
        ox, oy = (0, 0) if origins is None else (int(origins[f][0]), int(origins[f][1]))
        out.append((int(tag), int(f), int(a), int(labels[f]), ident, ox, oy))
    return out


def clamp_icon(icon, w, h):
    """imgproc.cpp:11-15 on one armour's icon [4, 2] float32: x into [0, w - 1], y into [0, h - 1], in float32 as the reference compares"""
    ic = np.asarray(icon, np.float32).reshape(4, 2).copy()
    lim = np.array([np.float32(w) - np.float32(1), np.float32(h) - np.float32(1)], np.float32)
    for i in range(4):
        for k in range(2):                                                    # std::max(0.0f, std::min(v, lim)), scalar by scalar:
            v = ic[i, k]
            t = lim[k] if lim[k] < v else v                                   # min(a, b): b when b < a, else a (a NaN stays)
            ic[i, k] = t if np.float32(0) < t else np.float32(0)              # max(a, b): b when a < b, else a (NaN and -0 give +0)
    return ic


def tables(n_frames, max_armours, seed, ovf_bits=True):
    """seeded tables of one append call: counts that are 0, 1, max_armours and beyond it; skip labels; each RMCV_FRAME_OVF_* bit and the
    informational bits (16, 32, 64: they change nothing); identities that match and miss the frame's label"""
    r = np.random.RandomState(seed)
    n = r.choice([0, 0, 1, 2, max_armours - 1, max_armours, max_armours + 1, max_armours + 7], n_frames).astype(np.int32)
    status = r.choice([0, 0, 0, 0, 16, 32, 64, 80] + ([1, 2, 4, 8, 9, 8 | 64] if ovf_bits else []), n_frames).astype(np.int32)
    labels = r.randint(0, 7, n_frames).astype(np.int32)
    labels[r.rand(n_frames) < 0.2] = SKIP
    identity = np.where(r.rand(n_frames, max_armours) < 0.5, labels[:, None], r.randint(0, 7, (n_frames, max_armours))).astype(np.int32)
    if n_frames >= 8:   # every special value at least once, whatever the seed
        n[:4] = [0, 1, max_armours, max_armours + 3]
        status[:8] = [0, 0, 0, 0, 1, 2, 4, 8]
        n[4:8] = 2
        labels[:8] = [1, 2, 3, 4, 1, 2, 3, 4]
    return n, status, labels, identity


def capacities(n, status, labels, identity, max_armours, flags):
    """(count, capacity) pairs for one call: room for everything; a capacity that falls before, inside and after a frame's rows; a dataset
    that is already full"""
    items, kept, _ = plan(n, status, labels, identity, max_armours, flags, 0, 1 << 30)
    out = [(0, kept + 5), (3, kept + 3 + 1), (7, 7), (0, 1)]
    if kept:
        frames, firsts = np.unique(items[:, 0], return_index=True)
        big = [i for i, f in enumerate(frames) if np.sum(items[:, 0] == f) >= 2]
        if big:
            at = int(firsts[big[len(big) // 2]])
            out += [(2, 2 + at), (2, 2 + at + 1), (2, 2 + at + int(np.sum(items[:, 0] == frames[big[len(big) // 2]])))]   # before, inside, after that frame's rows
    return out
