"""The calls tests/test_harvest_plan.py and tests/test_harvest_sanitized.py feed tests/harvest_san_main.cpp, and how its answer is read."""
import struct

import numpy as np

import harvest_ref as R

FRAMES = (1, 63, 64, 65, 256, 257, 1000)
MAX_ARMOURS = 6


def calls():
    """[(n, status, labels, identity, max_armours, flags, count, capacity, dropped)]: every frame count, both flag values, and for each the
    capacities of harvest_ref.capacities (room for all; before, inside, after a frame's rows; already full)"""
    out = []
    for n_frames in FRAMES:
        n, st, lb, ident = R.tables(n_frames, MAX_ARMOURS, 100 + n_frames)
        for flags in (0, R.MISSES):
            for count, capacity in R.capacities(n, st, lb, ident, MAX_ARMOURS, flags):
                out.append((n, st, lb, ident if flags or n_frames % 2 else None, MAX_ARMOURS, flags, count, max(capacity, count, 1), 11 * len(out)))
    return out


def encode(cs):
    b = struct.pack("<i", len(cs))
    for n, st, lb, ident, ma, flags, count, capacity, dropped in cs:
        b += struct.pack("<6iq", len(n), ma, flags, count, capacity, int(ident is not None), dropped)
        b += n.astype("<i4").tobytes() + st.astype("<i4").tobytes() + lb.astype("<i4").tobytes() + (b"" if ident is None else ident.astype("<i4").tobytes())
    return b


def decode(b, cs):
    """-> [(items [m, 3], count, dropped, kept_per_frame)] and checks that nothing is left over"""
    out, at = [], 0
    for c in cs:
        m, count, dropped = struct.unpack_from("<iiq", b, at)
        at += 16
        items = np.frombuffer(b, "<i4", 3 * m, at).reshape(m, 3)
        at += 12 * m
        per = np.frombuffer(b, "<i4", len(c[0]), at)
        at += 4 * len(c[0])
        out.append((items, count, dropped, per))
    assert at == len(b)
    return out


def check(got, cs):
    """the program's answers against the restatement: slots, count and dropped equal everywhere; and that the cases are what they claim"""
    seen = {"dropped": 0, "full": 0, "all": 0, "skip": 0, "ovf": set(), "beyond": 0, "miss_kept": 0, "miss_left": 0}
    for (items, count, dropped, per), (n, st, lb, ident, ma, flags, c0, cap, d0) in zip(got, cs):
        want_items, want_count, want_dropped = R.plan(n, st, lb, ident, ma, flags, c0, cap, d0)
        assert np.array_equal(items, want_items) and count == want_count and dropped == want_dropped, (len(n), flags, c0, cap)
        all_items, _, _ = R.plan(n, st, lb, ident, ma, flags, 0, 1 << 30)
        assert np.array_equal(per, np.bincount(all_items[:, 0], minlength=len(n)))
        assert np.array_equal(items, all_items[:len(items)] + [0, 0, c0])   # a full dataset holds a prefix of the unbounded one
        seen["dropped"] += dropped > d0
        seen["full"] += c0 == cap
        seen["all"] += dropped == d0 and len(items) > 0
        seen["skip"] += int(np.any(lb == R.SKIP))
        seen["ovf"] |= set(int(b) for b in (1, 2, 4, 8) if np.any(st & b))
        seen["beyond"] += int(np.any(n > ma))
        if flags:
            cand = np.arange(ma)[None, :] < np.where((lb != R.SKIP) & ((st & R.OVF) == 0), np.clip(n, 0, ma), 0)[:, None]
            seen["miss_kept"] += int(np.sum(cand & (ident != lb[:, None])))
            seen["miss_left"] += int(np.sum(cand & (ident == lb[:, None])))
    assert seen["dropped"] and seen["full"] and seen["all"] and seen["skip"] and seen["beyond"] and seen["ovf"] == {1, 2, 4, 8}
    assert seen["miss_kept"] and seen["miss_left"]
