"""The pose stage on the GPU, case for case (tests/pose_cases.py; the CPU side is tests/test_pose_cases_cpu.py): every case goes through every
route that reaches k_pnp -- rmcv_locate_armours in chunks of 1, 63, 64, 65 and max_armours; the batch's STAGE_POSE on injected armours with
per-frame counts 0, 1, 64, 65, max_armours and beyond; a camera table holding every configuration, selected per frame from the host and from
a device table with stray values; windows, whose origins are added to the vertices in float32.

Comparison rule: the device's rvec, tvec and position are the oracle's in raw bytes, with one exception -- a NaN matches any NaN (sign and
payload of a generated NaN differ between x86 and the GPU; the reference promises neither).  Every finite value, every zero's sign and every
Inf must match exactly.  The NaN outputs are counted and printed."""
import ctypes as C
import functools

import numpy as np
import pytest

import pose_cases as K
from rmcv_amd import STAGE_ALL, STAGE_POSE, Context, default_params, default_pnp_config
from rmcv_amd import abi
from rmcv_amd.abi import lib, ptr
from test_oracle_pnp import rodrigues

pytestmark = pytest.mark.gpu

NF, CAP = 16, 96                                                              # frames per batch (>= the configurations), armours per frame
SIDE = 64                                                                     # the frames (and the windows) are SIDE x SIDE
QUIET = dict(lower_bound=255)                                                 # a pixel pass that finds nothing: the armours are injected
COUNTS = (0, 1, 64, 65, CAP, CAP + 3)                                         # lane 0 alone, a full wavefront, one lane into the second trip, the cap, beyond
FRAME_W, FRAME_H = 800, 600                                                   # the frames of the window route
CHUNKS = (1, 63, 64, 65)                                                      # ... of rmcv_locate_armours, and the context's max_armours


@functools.lru_cache(maxsize=None)
def matrices():
    """NF base2gripper matrices: rigid ones, one holding a NaN, one holding -0 entries, the identity"""
    rng = np.random.default_rng(K.SEED + 1)
    m = np.tile(np.eye(4), (NF, 1, 1))
    for f in range(NF):
        m[f, :3, :3] = rodrigues(rng.uniform(-1, 1, 3))
        m[f, :3, 3] = rng.uniform(-50, 50, 3)
    m[3, 1, 2] = np.nan
    m[5] = np.eye(4)
    m[7] = np.full((4, 4), -0.0)                                              # -0 off the diagonal
    m[7][np.arange(4), np.arange(4)] = (1.0, -1.0, 1.0, 1.0)
    assert np.signbit(m[7, 0, 1]) and np.isnan(m[3]).any()
    m.setflags(write=False)
    return m


def armours_of(vertices):
    a = np.zeros(len(vertices), abi.ARMOUR)
    a["vertices"] = vertices
    return a


def compare(got, want, names, where, tally):
    """got, want: (rvec, tvec, position) triples of [n, 3]; tally: [rows compared, NaN values in the oracle's rows]"""
    for g, w, what in zip(got, want, ("rvec", "tvec", "position")):
        assert g.shape == w.shape, (where, what, g.shape, w.shape)
        bad = [names[i] for i in range(len(w)) if not K.same_bytes_but_nan(g[i], w[i])[0]]
        assert not bad, (where, what, bad[:8], len(bad))
        tally[1] += int(np.isnan(w).sum())
    tally[0] += len(want[0])


@pytest.fixture(scope="module")
def ocfgs(oracle):
    return {n: K.to_oracle_cfg(oracle, c) for n, c in K.configs().items()}


@pytest.fixture(scope="module")
def small():
    """a context of NF small frames with CAP armours each, shared by the batch routes"""
    c = Context(device=0, max_frames=NF, max_width=FRAME_W, max_height=FRAME_H, max_armours=CAP)
    yield c
    c.close()


def up(dst, src):
    assert lib().rmcv_device_upload(0, C.c_void_p(dst), ptr(src), C.c_int64(src.nbytes)) == 0


def bind_quiet(c, w=SIDE, h=SIDE, windows=None):
    """NF black frames bound and run through a pixel pass that finds nothing; windows: (origins, win_w, win_h)"""
    c.upload(np.zeros((NF, h, w, 3), np.uint8))
    if windows is not None:
        c.set_windows(*windows)
    c.run(default_params(**QUIET), STAGE_ALL)
    c.sync()
    k = c.counts()
    assert not k["n_armours"].any() and not k["status"].any()


def inject(c, per_frame, counts):
    """per_frame: the case indices of every frame's rows (at most CAP); counts: what the count table says (may exceed CAP)"""
    d_arm, d_cnt, cap, n = c.device_views()
    assert cap == CAP and n == NF
    table = np.zeros((NF, CAP), abi.ARMOUR)
    for f, idx in enumerate(per_frame):
        assert len(idx) == min(counts[f], CAP)
        table[f, :len(idx)]["vertices"] = K.vertices_of(idx)
    up(d_arm, table)
    up(d_cnt, np.asarray(counts, np.int32))
    return table


def rounds_of(indices, shift=0):
    """the cases `indices` dealt out to rounds of NF frames whose counts cycle through COUNTS (every frame full: the list wraps around)"""
    counts = [COUNTS[(f + shift) % len(COUNTS)] for f in range(NF)]
    room = sum(min(k, CAP) for k in counts)
    out = []
    for first in range(0, len(indices), room):
        per_frame, o = [], first
        for k in counts:
            k = min(k, CAP)
            per_frame.append([indices[(o + j) % len(indices)] for j in range(k)])
            o += k
        out.append((per_frame, counts))
    return out


def check_frames(c, oracle, per_frame, counts, cfg_of_frame, ocfgs, origins, where, tally):
    """the batch's getters against the oracle: min(count, CAP) rows per frame, in table order"""
    c.sync()
    arm, offs = c.armours()
    r, t, p = c.poses()
    rows = [min(k, CAP) for k in counts]
    assert offs.tolist() == np.concatenate([[0], np.cumsum(rows)]).tolist(), where
    assert len(r) == len(arm) == sum(rows), where
    names = [c_[0] for c_ in K.cases()]
    mats = matrices()
    for f, idx in enumerate(per_frame):
        sl = slice(offs[f], offs[f + 1])
        v = K.vertices_of(idx)
        assert arm[sl]["vertices"].tobytes() == v.tobytes(), (where, f)       # the table is only read
        if origins is not None:
            v = v + origins[f].astype(np.float32)                             # mobility.cpp:172, :182-185: added in float32
        want = oracle.locate_armours(armours_of(v), ocfgs[cfg_of_frame[f]], mats[f])
        compare((r[sl], t[sl], p[sl]), want, [names[i] for i in idx], (where, f), tally)


# ---------------------------------------------------------------- 1. rmcv_locate_armours
def test_locate_armours_every_case(ctx, oracle, ocfgs):
    cap = ctx.limits.max_armours
    names = [c[0] for c in K.cases()]
    mats = matrices()
    tally = [0, 0]
    used = set()
    try:
        for cname, idx in K.by_config().items():
            ctx.pnp_load(K.configs()[cname])
            o, k = 0, 0
            while o < len(idx):
                n = (CHUNKS + (cap,))[k % (len(CHUNKS) + 1)]
                chunk = [idx[(o + j) % len(idx)] for j in range(n)]           # (a chunk is always full: the list wraps around)
                arm = armours_of(K.vertices_of(chunk))
                for base in (None, mats[k % NF], mats[3], mats[7]):           # without, with, with a NaN, with -0 entries
                    compare(ctx.locate_armours(arm, base), oracle.locate_armours(arm, ocfgs[cname], base), [names[i] for i in chunk],
                            (cname, o, n), tally)
                used.add(n)
                o, k = o + n, k + 1
    finally:
        ctx.pnp_load(default_pnp_config())
    print("rmcv_locate_armours: %d rows compared, %d NaN values among the oracle's" % tuple(tally))
    assert used == set(CHUNKS) | {cap} and tally[0] >= 4 * len(names) and tally[1] > 0


# ---------------------------------------------------------------- 2. the batch stage on injected armours
def test_batch_pose_stage_on_injected_armours(small, oracle, ocfgs):
    c = small
    c.pnp_load()
    bind_quiet(c)
    c.set_base2gripper(matrices())
    tally, seen = [0, 0], set()
    for k, (cname, idx) in enumerate(K.by_config().items()):
        c.pnp_load(K.configs()[cname])
        for per_frame, counts in rounds_of(idx, shift=k):
            inject(c, per_frame, counts)
            c.run(default_params(**QUIET), STAGE_POSE)                        # alone: the table stays the injected one
            check_frames(c, oracle, per_frame, counts, [cname] * NF, ocfgs, None, cname, tally)
            assert c.counts()["n_armours"].tolist() == list(counts)           # (the count table itself is the caller's, unclamped)
            seen |= {i for fr in per_frame for i in fr}
    print("STAGE_POSE on injected armours: %d rows compared, %d NaN values among the oracle's" % tuple(tally))
    assert seen == set(range(len(K.cases()))) and tally[1] > 0


# ---------------------------------------------------------------- 3. the camera table
STRAY = (-1, 1000, -2**31, 2**31 - 1, -7, 15, 16)


def test_camera_table_serves_every_configuration(small, oracle, ocfgs):
    """every configuration in one table; round r gives frame f the configuration (f + r) mod the table's length -- from the host's indices in
    even rounds, from a device table with stray values in odd ones -- and the next rows of that configuration's cases, its first ones first
    (the named ones, which take its special branch), until every case has been in a frame"""
    c = small
    names = list(K.configs())
    by = K.by_config()
    assert len(names) <= NF
    cursor = {n: 0 for n in names}
    tally, seen, served, strays = [0, 0], set(), set(), 0
    d_idx = C.c_void_p()
    assert lib().rmcv_device_alloc(0, C.c_int64(4 * NF), C.byref(d_idx)) == 0
    try:
        c.pnp_load_cameras([K.configs()[n] for n in names])
        bind_quiet(c)
        c.set_base2gripper(matrices())
        r = 0
        while len(seen) < len(K.cases()):
            assert r < 80
            raw = np.array([(f + r) % len(names) for f in range(NF)], np.int32)
            if r % 2 == 0:                                                    # the host's indices: validated, inside the table
                c.set_frame_cameras(raw)
            else:                                                             # a device table, borrowed, any values
                raw[1::4] = [STRAY[(r + j) % len(STRAY)] for j in range(len(raw[1::4]))]
                up(d_idx.value, raw)
                c.set_frame_cameras(int(d_idx.value))
            eff = np.array([c.frame_camera(int(i), len(names)) for i in raw], np.int32)
            assert eff.min() >= 0 and eff.max() < len(names)
            strays += int((eff != raw).sum())
            counts = [COUNTS[(f + r) % len(COUNTS)] for f in range(NF)]
            per_frame = []
            for f in range(NF):
                n = names[eff[f]]
                rows = min(counts[f], CAP)
                per_frame.append([by[n][(cursor[n] + j) % len(by[n])] for j in range(rows)])
                cursor[n] += rows
            inject(c, per_frame, counts)
            c.run(default_params(**QUIET), STAGE_POSE)
            check_frames(c, oracle, per_frame, counts, [names[e] for e in eff], ocfgs, None, ("round", r), tally)
            assert np.array_equal(c.frame_cameras(), eff), r
            seen |= {i for fr in per_frame for i in fr}
            served |= {names[eff[f]] for f in range(NF) if per_frame[f]}
            c.set_frame_cameras(None)
            r += 1
    finally:
        c.set_frame_cameras(None)
        lib().rmcv_device_free(0, d_idx)
        c.pnp_load()
    print("camera table: %d rounds, %d rows compared, %d NaN values among the oracle's, %d stray indices" % (r, tally[0], tally[1], strays))
    assert served == set(names) and r >= 2 and strays > 0 and tally[1] > 0


# ---------------------------------------------------------------- 4. windows
def test_windows_add_their_origin_in_float32(small, oracle, ocfgs):
    c = small
    rng = np.random.default_rng(K.SEED + 2)
    origins = np.stack([16 * rng.integers(19, (FRAME_W - SIDE) // 16, NF), rng.integers(200, FRAME_H - SIDE, NF)], axis=1).astype(np.int32)
    c.pnp_load()
    tally, seen, rounded = [0, 0], set(), 0
    try:
        bind_quiet(c, FRAME_W, FRAME_H, (origins, SIDE, SIDE))
        eff, ww, wh = c.windows()
        assert (ww, wh) == (SIDE, SIDE) and np.array_equal(eff, origins) and (eff >= 200).all()    # effective as they are, none zero
        c.set_base2gripper(matrices())
        for k, (cname, idx) in enumerate(K.by_config().items()):
            c.pnp_load(K.configs()[cname])
            for per_frame, counts in rounds_of(idx, shift=k + 2):
                inject(c, per_frame, counts)
                c.run(default_params(**QUIET), STAGE_POSE)
                check_frames(c, oracle, per_frame, counts, [cname] * NF, ocfgs, eff, ("windows", cname), tally)
                for f, fr in enumerate(per_frame):
                    v = K.vertices_of(fr)
                    if len(v):
                        exact = v.astype(np.float64) + eff[f]
                        with np.errstate(invalid="ignore"):
                            moved = (v + eff[f].astype(np.float32)).astype(np.float64)
                        rounded += int((np.isfinite(exact) & (moved != exact)).any(axis=(1, 2)).sum())
                seen |= {i for fr in per_frame for i in fr}
        # the stage-wise call keeps the default ROI whatever windows the context has
        some = K.by_config()["default"][:CAP]
        arm = armours_of(K.vertices_of(some))
        c.pnp_load()
        compare(c.locate_armours(arm), oracle.locate_armours(arm, ocfgs["default"], None), [K.cases()[i][0] for i in some], "stage-wise", tally)
    finally:
        c.set_windows(None, 0, 0)
        c.pnp_load()
    print("windows: %d rows compared, %d NaN values among the oracle's, vertex + origin rounded in float32 for %d rows" % (tally[0], tally[1], rounded))
    assert seen == set(range(len(K.cases()))) and tally[1] > 0
    assert rounded >= 300                                                     # fractional vertices beside origins of several hundred
