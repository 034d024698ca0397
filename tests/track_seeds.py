"""Seeded cases for every branch of the device tracker's step (tests/test_tracker_seeds_cpu.py, tests/test_gpu_tracker_seeds.py).  No GPU.

The association depends only on armour.bbox and lost_count of the current list, so a list seeded (rmcv_tracker_put) with boxes placed ON,
NEAR or AWAY from the boxes a fixed frame really yields steers every branch: nothing has to be rendered.  A seed is a DONOR track -- a
valid filter state taken from the hypot-pinned reference's run over tests/track_scenarios.py -- with armour.bbox, armour.vertices (and
the side record), lost_count, timestamp and the identity histogram overwritten.  A case is a frame, a tracker group (one tracker
configuration, one batch), a builder (observed armours in FRAME coordinates, identities, the step's timestamp) -> (tracks, side) and
the branch census its first step must reach; Stream.step computes that census on the reference alone (RefStream._walk and the outcome).

Frames (1280 x 1024 BGR, camp blue), with the armour counts of the CPU oracle:
  plain   synth.frame(i)                                        1 .. 8   (1: 1 armour, 5: 2, 2: 3, 3: 6)
  tile4   2 x 2 tiling of synth.frame(first + c, 640, 512)      20 / 18 / 18 for first = 0 / 16 / 32
  tile16  4 x 4 tiling of synth.frame(first + c, 320, 256)      107 / 109 / 92
  black   zeros                                                 none
Windows (requested origin -> effective origin, armours of the crop): 26 @ (1001, 500) -> (768, 500): 3; 46 @ (213, 100) -> (208, 100): 6;
3 @ (485, 700) -> (480, 640): 2; 54 @ (213, 450) -> (208, 450): 5.  Every requested x is no multiple of 16, two origins lie partly
outside the frame: the effective origin is clamped and snapped, ob.fx and ob.fy are non-zero."""
import functools
from collections import namedtuple

import numpy as np

import track_ref as T
import track_scenarios as S
from rmcv_amd import CAMP_BLUE, abi, synth
from rmcv_amd.tracker import Tracker, default_tracker_config

FW, FH, WW, WH = 1280, 1024, 512, 384
MS = 1_000_000
STAMPS = (20_000 * MS, 20_008 * MS, 20_019 * MS)     # the three chained steps (tick_frequency 1e9)
ORIGIN0 = (37, -5)                                    # what set_origins writes before the first step
TRACK, ARMOUR = abi.TRACK, abi.ARMOUR

# tracker groups: one tracker (and one batch) each.  whole: the batch reads whole frames (fine for a windowed tracker: the host decides per
# batch -- the origin is still written); otherwise through host windows of WW x WH at the cases' requested origins
Group = namedtuple("Group", "config whole")
GROUPS = {
    "full": Group(dict(track_cap=64, win_w=WW, win_h=WH), True),
    "win": Group(dict(track_cap=64, win_w=WW, win_h=WH), False),
    "roi": Group(dict(track_cap=64, win_w=WW, win_h=WH, roi_scale_w=1.5, roi_scale_h=2.0), False),
    "cap4": Group(dict(track_cap=4, win_w=WW, win_h=WH), True),
    "cap1": Group(dict(track_cap=1, win_w=WW, win_h=WH), True),
    "bare": Group(dict(track_cap=64), True),
}


def config(group, **kw):
    return default_tracker_config(frame_w=FW, frame_h=FH, **dict(GROUPS[group].config, **kw))


# ---------------------------------------------------------------- frames
def _tile(first, g):
    w, h = FW // g, FH // g
    out = np.zeros((FH, FW, 3), np.uint8)
    for c in range(g * g):
        r, q = divmod(c, g)
        out[r * h:(r + 1) * h, q * w:(q + 1) * w] = synth.frame(first + c, w, h, CAMP_BLUE)
    return out


@functools.lru_cache(maxsize=None)
def frame(key):
    """key: ("plain", i) | ("tile4", first) | ("tile16", first) | ("black",)"""
    if key[0] == "plain":
        f = synth.frame(key[1], FW, FH, CAMP_BLUE)
    elif key[0] == "black":
        f = np.zeros((FH, FW, 3), np.uint8)
    else:
        f = _tile(key[1], {"tile4": 2, "tile16": 4}[key[0]])
    f.setflags(write=False)
    return f


BLACK = ("black",)


# ---------------------------------------------------------------- donors
@functools.lru_cache(maxsize=None)
def donors():
    """valid filter states from the reference's own run of the CPU scenarios: hist (initialised, with history), new (initialized == 0:
    straight after a fresh observation), nan (equal_stamps after step 20: dt = 0 on a matched update)"""
    def lists(name, at):
        over, steps = S.scenarios()[name]
        cfg = default_tracker_config(frame_w=FW, frame_h=FH, **over)
        ref = T.RefStream(T.lib(), cap=cfg.track_cap, tick=cfg.tick_frequency, noise=(cfg.process_noise, cfg.measurement_noise, cfg.error),
                          roi_scale=(cfg.roi_scale_w, cfg.roi_scale_h), frame=(FW, FH), win=(cfg.win_w, cfg.win_h))
        out = {}
        for k, (arm, ids, pos, ts) in enumerate(steps[:max(at) + 1]):
            assert ref.step(arm, ids, pos, ts)
            if k in at:
                out[k] = ref.tracks.copy()
        return out
    st, cr, idn, dr, eq = lists("static", (0, 40)), lists("crossing", (30,)), lists("identities", (60,)), lists("drift", (50,)), lists("equal_stamps", (25,))
    hist = np.concatenate([st[40], cr[30], idn[60], dr[50]])
    hist = hist[hist["initialized"] == 1]
    new, nan = st[0], eq[25]
    assert len(hist) >= 6 and np.isfinite(hist["state_post"]).all() and (hist["n_ids"] >= 1).all()
    assert len(new) == 1 and new[0]["initialized"] == 0
    assert len(nan) >= 1 and nan[0]["initialized"] == 1 and not np.isfinite(nan[0]["state_post"]).all()
    return dict(hist=hist, new=new[0], nan=nan[0])


def box_vertices(box):
    x, y, w, h = (float(v) for v in box)
    return np.array([[x, y + h], [x, y], [x + w, y], [x + w, y + h]], np.float32)


def iou(a, b):
    """plain intersection over union of two (x, y, w, h) boxes (only to place seeds: far from 0.5 on either side)"""
    iw = min(a[0] + a[2], b[0] + b[2]) - max(a[0], b[0])
    ih = min(a[1] + a[3], b[1] + b[3]) - max(a[1], b[1])
    inter = max(float(iw), 0.0) * max(float(ih), 0.0)
    union = float(a[2]) * float(a[3]) + float(b[2]) * float(b[3]) - inter
    return inter / union if union > 0 else 0.0


class Seeds:
    """the list under construction: add(donor, ...) appends one seed"""

    def __init__(self, arm, ts):
        self.arm, self.ts, self.tracks, self.side = arm, int(ts), [], []
        self.D = donors()

    def hist(self, k):
        h = self.D["hist"]
        return h[k % len(h)]

    def add(self, donor, box, lost=0, ts=None, verts=None, ids=None):
        t = np.zeros(1, TRACK)
        t[0] = donor
        v = box_vertices(box) if verts is None else np.asarray(verts, np.float32)
        t["armour"]["bbox"][0] = box
        t["armour"]["vertices"][0] = v
        t["lost_count"], t["timestamp"] = lost, (self.ts - (8 + len(self.tracks) % 5) * MS if ts is None else int(ts))
        if ids is not None:
            ids = [int(i) for i in ids]
            assert ids == sorted(set(ids)) and len(ids) <= abi.TRACK_IDS
            t["n_ids"], t["ids"], t["counts"] = len(ids), 0, 0
            t["ids"][0, :len(ids)] = ids
            t["counts"][0, :len(ids)] = [1 + (q * 3) % 5 for q in range(len(ids))]
        self.tracks.append(t[0])
        self.side.append(v)

    def match(self, donor, k, shift=0.0, **kw):
        """a seed ON observation k (shift: NEAR it, moved by that share of the width)"""
        b = self.arm[k]["bbox"].copy()
        if shift:
            b[0] += np.float32(np.floor(shift * b[2]))
            assert iou(b, self.arm[k]["bbox"]) > 0.6
            self.add(donor, b, **kw)
        else:
            self.add(donor, b, verts=self.arm[k]["vertices"], **kw)

    def away(self, donor, slot, zero_width=False, **kw):
        """a seed AWAY from every observation: a small box on a grid inside the frame"""
        b = np.array([8 + 19 * (slot % 64), 9 + 15 * (slot // 64) + 11 * (slot % 7), 0 if zero_width else 5, 4], np.float32)
        assert all(iou(b, a["bbox"]) < 0.25 for a in self.arm)
        self.add(donor, b, **kw)

    def done(self):
        if not self.tracks:
            return np.zeros(0, TRACK), np.zeros((0, 4, 2), np.float32)
        return np.array(self.tracks, TRACK), np.array(self.side, np.float32).reshape(-1, 4, 2)


# ---------------------------------------------------------------- builders: (armours in frame coordinates, identities, timestamp) -> (tracks, side)
def b_empty(arm, ids, ts):
    return Seeds(arm, ts).done()


def b_many_match(arm, ids, ts):
    """one initialised seed ON every observation, the list in a fixed permutation of the observations' order"""
    s = Seeds(arm, ts)
    for j, k in enumerate(np.random.default_rng(7).permutation(len(arm))):
        s.match(s.hist(j), int(k), lost=j % 3)
    return s.done()


def overlapping_pair(arm):
    """the first two observations whose boxes overlap with IoU > 0.6 (the tiles have some), or None"""
    for i in range(len(arm)):
        for j in range(len(arm)):
            if i != j and iou(arm[i]["bbox"], arm[j]["bbox"]) > 0.6:
                return i, j
    return None


def b_mixed(arm, ids, ts):
    """about 40 seeds on a tile4 frame: every action, erasures next to each other and in the last slot, the erase-skip in front of a seed
    that would have matched, a zero-width box, two seeds competing for one observation"""
    n = len(arm)
    assert 9 <= n <= 40
    s = Seeds(arm, ts)
    pair = overlapping_pair(arm)
    taken = set()
    if pair:                                 # two seeds ON the same observation: the first takes it, the second its overlapping neighbour
        s.match(s.hist(0), pair[0])
        s.match(s.hist(1), pair[0], lost=3)
        taken |= set(pair)
    free = [k for k in range(n) if k not in taken]
    s.away(s.hist(2), 0, lost=0)
    s.match(s.hist(3), free[0])
    s.away(s.hist(4), 1, lost=26)            # erased ...
    s.away(s.hist(5), 2, lost=27)            # ... its neighbour moves into the slot and is skipped: kept, although it is as old
    s.away(s.hist(6), 3, lost=1000)          # erased: two erasures in consecutive passes of the walk
    s.match(s.hist(7), free[1])              # kept untouched: observation free[1] becomes fresh
    s.match(s.hist(8), free[2], shift=0.1)   # NEAR
    s.away(s.hist(9), 4, lost=1)
    s.away(s.hist(10), 5, lost=25)           # the 26th miss: coasts once more
    s.away(s.hist(11), 6, lost=25, zero_width=True)
    s.away(s.D["new"], 7, lost=2)
    for j, k in enumerate(free[3:8]):
        s.match(s.hist(12 + j), k, lost=j)
    s.away(s.hist(17), 8, lost=26)           # erased; the next one is kept
    s.away(s.hist(18), 9, lost=0)
    for j in range(40 - len(s.tracks) - 2):
        s.away(s.hist(19 + j), 10 + j, lost=j % 26)
    s.away(s.hist(3), 62, lost=5)
    s.away(s.hist(4), 63, lost=27)           # an erasure in the last slot
    return s.done()


def b_cap(total):
    """three matches and as many coasting seeds as make survivors + fresh exactly `total`"""
    def build(arm, ids, ts):
        n = len(arm)
        assert 9 <= n <= 40
        s = Seeds(arm, ts)
        for k in range(3):
            s.match(s.hist(k), k)
        for j in range(total - n):
            s.away(s.hist(3 + j), j, lost=j % 26)
        assert len(s.tracks) <= 64
        return s.done()
    return build


def b_flood(n_seeds, n_match=0):
    def build(arm, ids, ts):
        n = len(arm)
        assert 65 <= n <= 128                       # TRK_MAX_OBS; the context's max_armours is 256
        s = Seeds(arm, ts)
        for k in range(n_match):
            s.match(s.hist(k), 5 * k)
        for j in range(n_seeds - n_match):
            s.away(s.hist(j), j, lost=j % 26)
        return s.done()
    return build


def b_coasters(n_seeds):
    def build(arm, ids, ts):
        s = Seeds(arm, ts)
        for j in range(n_seeds):
            s.away(s.hist(j), j, lost=j)
        return s.done()
    return build


def b_cap4_applied(arm, ids, ts):
    """two matches + one coasting seed + one fresh observation = 4"""
    assert len(arm) == 3
    s = Seeds(arm, ts)
    s.match(s.hist(0), 2)
    s.away(s.hist(1), 0, lost=4)
    s.match(s.hist(2), 0)
    return s.done()


def b_match_first(arm, ids, ts):
    s = Seeds(arm, ts)
    s.match(s.hist(0), 0)
    return s.done()


def _ids_around(i, where):
    """31 ascending identities without `i`, which would sort first / in the middle / last"""
    return {"first": list(range(i + 1, i + 32)), "middle": list(range(i - 15, i)) + list(range(i + 1, i + 17)), "last": list(range(i - 31, i))}[where]


def b_identities(arm, ids, ts):
    """every seed ON an observation: a full histogram WITH the observed identity (counts++), 31 entries and the observed one sorting first,
    in the middle, last (the insertion keeps ids ascending)"""
    assert len(arm) >= 4 and ids is not None
    s = Seeds(arm, ts)
    i = int(ids[0])
    s.match(s.hist(0), 0, ids=list(range(i - 20, i + 12)))
    for k, where in ((1, "first"), (2, "middle"), (3, "last")):
        s.match(s.hist(k), k, ids=_ids_around(int(ids[k]), where))
    return s.done()


def b_identities_refused(arm, ids, ts):
    """as b_identities, and one seed whose full histogram lacks the observed identity: the 33rd -- the whole step is refused"""
    assert len(arm) >= 5 and ids is not None
    tr, side = b_identities(arm, ids, ts)
    s = Seeds(arm, ts)
    i = int(ids[4])
    s.match(s.hist(4), 4, ids=[q for q in range(i - 16, i + 17) if q != i])
    t2, s2 = s.done()
    return np.concatenate([tr, t2]), np.concatenate([side, s2])


def b_stamps(arm, ids, ts):
    """matching seeds stamped with the step's time (dt = 0: NaN), 3 ms after it (negative dt), 10 s before it; NaN-state and
    initialized == 0 donors that match and that coast"""
    assert len(arm) >= 5
    s = Seeds(arm, ts)
    s.match(s.hist(0), 0, ts=ts)
    s.match(s.hist(1), 1, ts=ts + 3 * MS)
    s.match(s.hist(2), 2, ts=ts - 10_000 * MS)
    s.match(s.D["nan"], 3)
    s.away(s.D["nan"], 0, lost=1)
    s.match(s.D["new"], 4)
    s.away(s.D["new"], 1, lost=0)
    return s.done()


def b_win_mixed(arm, ids, ts):
    """the small mix for a window's two or three observations: NEAR match, coast, erase + keep (its observation becomes fresh), the 26th
    miss, an erasure in the last slot"""
    assert len(arm) >= 2
    s = Seeds(arm, ts)
    s.match(s.hist(0), 0, shift=0.1)
    s.away(s.hist(1), 0, lost=0)
    s.away(s.hist(2), 1, lost=26)
    s.match(s.hist(3), len(arm) - 1)
    s.away(s.hist(4), 2, lost=25)
    s.away(s.hist(5), 3, lost=27)
    return s.done()


def b_silent(arm, ids, ts):
    """no observation: nothing ages, nothing flips; the origin is rewritten from the newest seed -- two share the greatest timestamp, the
    lower index wins"""
    assert len(arm) == 0
    s = Seeds(arm, ts)
    s.add(s.hist(0), (300, 200, 60, 50), lost=3, ts=ts - 5 * MS)
    s.add(s.hist(1), (900, 610, 80, 40), lost=26, ts=ts - 1 * MS)
    s.add(s.D["nan"], (100, 800, 50, 50), lost=0, ts=ts - 1 * MS)
    return s.done()


# ---------------------------------------------------------------- the census of a case's first step
def c_many_match(c):
    assert c["applied"] and c["matches"] >= 9 and c["n_out"] >= 9 and c["matches"] == c["n_in"]


def c_many_fresh(c):
    assert c["applied"] and c["fresh"] >= 9 and c["n_out"] == c["fresh"] and c["n_in"] == 0


def c_mixed(c):
    assert c["applied"] and 38 <= c["n_in"] <= 40
    assert c["matches"] >= 7 and c["coast"] >= 10 and c["keep"] >= 3 and c["fresh"] >= 1 and c["erased"] >= 4 and c["n_out"] >= 17


def c_cap_exact(c):
    assert c["applied"] and c["n_out"] == 64 and c["matches"] == 3 and c["coast"] >= 24


def c_refused(c):
    assert c["refused"] and not c["applied"] and c["n_out"] == c["n_in"]


def c_cap_plus_one(c):
    c_refused(c)
    assert c["n_in"] - c["erased"] + c["fresh"] == 65 and c["n_obs"] <= c["n_in"] + 64


def c_flood_early(c):
    c_refused(c)
    assert c["n_obs"] > c["n_in"] + c["cap"]                  # refused in front of the walk


def c_flood_walk(c):
    c_refused(c)
    assert c["n_obs"] <= c["n_in"] + c["cap"] and c["n_in"] - c["erased"] + c["fresh"] > c["cap"]    # walked, then refused


def c_cap4_applied(c):
    assert c["applied"] and c["n_out"] == 4 and c["matches"] == 2 and c["coast"] == 1 and c["fresh"] == 1


def c_cap1_applied(c):
    assert c["applied"] and c["n_out"] == 1 and c["matches"] == 1 and c["n_obs"] == 1


def c_identities(c):
    assert c["applied"] and c["matches"] == 4 and c["n_ids_after"][:4] == [32, 32, 32, 32] and c["ids_ascending"]


def c_identities_refused(c):
    c_refused(c)
    assert c["matches"] == 5 and c["n_in"] - c["erased"] + c["fresh"] <= c["cap"]     # not the capacity: the 33rd identity


def c_stamps(c):
    assert c["applied"] and c["matches"] == 5 and c["coast"] == 2 and c["nan_after"] >= 3      # dt = 0 and both NaN donors


def c_win_mixed(c):
    assert c["applied"] and c["matches"] >= 1 and c["coast"] >= 2 and c["keep"] >= 1 and c["erased"] >= 2 and c["fresh"] >= 1


def c_silent(c):
    assert not c["applied"] and not c["refused"] and c["n_obs"] == 0 and c["n_out"] == c["n_in"] == 3 and c["unchanged"]


Case = namedtuple("Case", "name group frame request build check")

CASES = [
    # whole frames into a windowed tracker of cap 64
    Case("many_match", "full", ("tile4", 0), None, b_many_match, c_many_match),
    Case("many_fresh", "full", ("tile4", 16), None, b_empty, c_many_fresh),
    Case("mixed", "full", ("tile4", 0), None, b_mixed, c_mixed),
    Case("cap_exact", "full", ("tile4", 32), None, b_cap(64), c_cap_exact),
    Case("cap_plus_one", "full", ("tile4", 32), None, b_cap(65), c_cap_plus_one),
    Case("flood_early_0", "full", ("tile16", 0), None, b_empty, c_flood_early),
    Case("flood_early_2", "full", ("tile16", 16), None, b_flood(2, 1), c_flood_early),
    Case("flood_walk", "full", ("tile16", 32), None, b_flood(64, 10), c_flood_walk),
    Case("identities", "full", ("plain", 3), None, b_identities, c_identities),
    Case("identities_refused", "full", ("plain", 3), None, b_identities_refused, c_identities_refused),
    Case("stamps", "full", ("plain", 3), None, b_stamps, c_stamps),
    # host windows: the requested x no multiple of 16, origins partly outside the frame
    Case("win_mixed", "win", ("plain", 26), (1001, 500), b_win_mixed, c_win_mixed),
    Case("win_silent", "win", BLACK, (485, 700), b_silent, c_silent),
    Case("win_stamps", "win", ("plain", 46), (213, 100), b_stamps, c_stamps),
    # ... and roi_scale (1.5, 2.0): trk_get_roi's scaled branch and its clamps
    Case("roi_mixed", "roi", ("plain", 3), (485, 700), b_win_mixed, c_win_mixed),
    Case("roi_silent", "roi", BLACK, (-37, 700), b_silent, c_silent),
    Case("roi_stamps", "roi", ("plain", 54), (213, 450), b_stamps, c_stamps),
    # track_cap 4 and 1: refused in front of the walk, refused behind it, applied
    Case("cap4_early", "cap4", ("plain", 3), None, b_empty, c_flood_early),
    Case("cap4_walk", "cap4", ("plain", 3), None, b_coasters(2), c_flood_walk),
    Case("cap4_applied", "cap4", ("plain", 2), None, b_cap4_applied, c_cap4_applied),
    Case("cap1_early", "cap1", ("plain", 3), None, b_match_first, c_flood_early),
    Case("cap1_walk", "cap1", ("plain", 5), None, b_match_first, c_flood_walk),
    Case("cap1_applied", "cap1", ("plain", 1), None, b_match_first, c_cap1_applied),
    # win_w == 0: the origin stays what set_origins wrote
    Case("bare", "bare", ("tile4", 16), None, b_mixed, c_mixed),
]
REFUSED = {c.name for c in CASES if c.check in (c_refused, c_cap_plus_one, c_flood_early, c_flood_walk, c_identities_refused)}


def group_cases(group):
    return [c for c in CASES if c.group == group]


def effective_origin(case):
    """the clamp and snap of the case's requested window origin; (0, 0) for whole frames"""
    if case.request is None:
        return 0, 0
    x = min(max(case.request[0], 0), FW - WW) & ~15
    y = min(max(case.request[1], 0), FH - WH)
    return x, y


Obs = namedtuple("Obs", "armours identities positions eff")   # armours in WINDOW coordinates with effective origin eff


class Stream:
    """one case's stream on the CPU: the seeded RefStream and, beside it, rmcv_tracker_step_host on the same inputs; every step asserts
    that the two are byte-equal and returns the census of the step, computed on the reference alone"""

    def __init__(self, case, origin=ORIGIN0):
        self.case, self.cfg = case, config(case.group)
        c = self.cfg
        self.ref = T.RefStream(T.lib(), cap=c.track_cap, tick=c.tick_frequency, noise=(c.process_noise, c.measurement_noise, c.error),
                               roi_scale=(c.roi_scale_w, c.roi_scale_h), frame=(FW, FH), win=(c.win_w, c.win_h), origin=origin)
        self.host = (np.zeros(0, TRACK), np.zeros((0, 4, 2), np.float32), 0, self.ref.origin)

    def put(self, tracks, side):
        assert len(tracks) <= self.cfg.track_cap
        self.ref.tracks, self.ref.side = tracks.copy(), side.copy()
        self.host = (tracks.copy(), side.copy(), self.host[2], self.host[3])

    def seed(self, obs, ts):
        """the case's list for these observations"""
        return self.case.build(abi.armours_to_frame(obs.armours, *obs.eff), obs.identities, ts)

    def state(self):
        r = self.ref
        return r.tracks.tobytes(), r.side.tobytes(), r.status, r.origin

    def step(self, obs, ts):
        r = self.ref
        arm = abi.armours_to_frame(obs.armours, *obs.eff)
        before, n_in = r.tracks.copy(), len(r.tracks)
        was = self.state()
        o = T.observations(r.L, arm, obs.identities, obs.positions, ts, r.noise)
        if len(o) and n_in:
            src, matched, left = r._walk(o)
        else:
            src, matched, left = list(range(n_in)), {}, list(range(len(o)))
        ok = r.step(arm, obs.identities, obs.positions, ts)
        c = dict(cap=self.cfg.track_cap, n_obs=len(o), n_in=n_in, refused=not ok, applied=bool(ok and len(o)), matches=len(matched),
                 erased=n_in - len(src), fresh=len(left), n_out=len(r.tracks), coast=0, keep=0)
        if c["applied"]:
            assert c["n_out"] == len(src) + len(left)
            for j, t in enumerate(src):
                if t in matched:
                    assert int(r.tracks[j]["timestamp"]) == ts
                elif r.tracks[j].tobytes() == before[t].tobytes():
                    c["keep"] += 1
                else:
                    assert int(r.tracks[j]["lost_count"]) == int(before[t]["lost_count"]) + 1
                    c["coast"] += 1
            for j in range(len(left)):
                assert int(r.tracks[len(src) + j]["initialized"]) == 0
        c["unchanged"] = self.state()[:2] == was[:2]
        assert c["applied"] or (c["unchanged"] and (self.state()[3] == was[3] or not c["refused"]))    # refused: not one byte moves
        assert r.status == (T.TRACKER_OVF if c["refused"] else 0) | was[2]                             # ... and the flag is sticky
        c["n_ids_after"] = [int(v) for v in r.tracks["n_ids"]]
        c["ids_ascending"] = all((np.diff(t["ids"][:int(t["n_ids"])]) > 0).all() for t in r.tracks)
        c["nan_after"] = sum(1 for t in r.tracks if not np.isfinite(t["state_post"]).all())
        # the product on the CPU: the source the kernel is compiled from
        self.host = Tracker.step_host(self.cfg, *self.host, obs.armours, obs.identities, obs.positions, obs.eff, ts)
        tr, side, st, org = self.host
        assert len(tr) == len(r.tracks) and st == r.status and org == r.origin, (self.case.name, len(tr), len(r.tracks), st, r.status, org, r.origin)
        assert tr.tobytes() == r.tracks.tobytes() and side.tobytes() == r.side.tobytes(), self.case.name
        return c
