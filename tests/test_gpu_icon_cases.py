"""The icon path on the GPU, branch for branch (tests/icon_cases.py; the CPU side is tests/test_icon_cases_cpu.py): every case goes through
every instantiation of icon_row (BGR, Bayer D(m), gamma table E(f), windows) and every consumer -- rmcv_classify_armours, the batch classifier
(k_classify*), the model table (k_classify_models), the dataset harvest (k_harvest_rows), the novelty append (k_novelty) and the fused tail of
the sparse kernel -- and every vote case through svm_predict, DeviceDataset.predict, the classifier kernels and (those with a finite rho: the
model table refuses the others) svm_predict(model=k).
Everything is compared with the oracle on the image that instantiation sees, in raw bytes: icons, identities and the armour table after the
in-place clamp.  No tolerance anywhere; the only conditions are coverage ones."""
import ctypes as C
import functools

import numpy as np
import pytest

import bayer_ref as BR
import enhance_ref as ER
import icon_cases as K
import model_ref as MR
import novelty_ref as NR
import raw_ref as RR
from rmcv_amd import STAGE_ALL, STAGE_IDENTITY, Context, DeviceDataset, default_params, synth
from rmcv_amd import abi
from rmcv_amd.abi import lib, ptr

pytestmark = pytest.mark.gpu

N, CAP = 8, 64                                                                # frames per batch, armours per frame
QUIET = dict(lower_bound=255)                                                 # a pixel pass that finds nothing: the armours are injected
BAYER8 = {"rg": BR.RG, "gb": BR.GB, "gr": BR.GR, "bg": BR.BG}
RAW12 = dict(pattern=BR.GB, bits=16, valid_bit=4, mirror=True, flip=True)
VARIANTS = ["bgr", "rg", "gb", "gr", "bg", "raw12", "enh", "win"]
BY_NAME = {c[0]: c for c in K.vote_cases()}
MODEL = K.model_of(BY_NAME["edge_2_8_mixed"])                                 # 8 classes, full-mantissa weights: identities vary over the list
TABLE = ["edge_2_8_mixed", "edge_0_2_mixed", "edge_1_4_above", "winner_3", "tie_all_5", "signs_3_-+-", "tie_two_4_later", "pattern_6_1"]
MODEL_IDX = np.array([1, 0, 2, 3, 4, 5, 7, 2], np.int32)


def finite(name):
    return bool(np.isfinite(BY_NAME[name][2]).all())


TABLE = [t if finite(t) else "winner_5" for t in TABLE]                       # (the model table refuses a rho that is not finite)


@functools.lru_cache(maxsize=None)
def frames():
    """eight different frames: the scene rolled sideways by 6 k pixels (an even step: the mosaics keep their pattern)"""
    f = np.stack([np.roll(K.frame(), 6 * k, axis=1) for k in range(N)])
    f.setflags(write=False)
    return f


def armours_of(icons):
    a = np.zeros(len(icons), abi.ARMOUR)
    for i, q in enumerate(icons):
        a[i]["icon"] = q
        a[i]["vertices"] = np.arange(8, dtype=np.float32).reshape(4, 2) + i    # (something to find untouched afterwards)
    return a


@functools.lru_cache(maxsize=None)
def material(variant):
    """what a variant uploads, what the oracle sees of each frame, the extent the icons are clamped to and the armours of every frame"""
    fr = frames()
    size = (K.WIN_W, K.WIN_H) if variant == "win" else (K.W, K.H)
    if variant in BAYER8:
        upload = BR.mosaic(fr, BAYER8[variant])
        images = [BR.demosaic(upload[f], BAYER8[variant]) for f in range(N)]
    elif variant == "raw12":
        dp = RR.derived_pattern(RAW12["pattern"], K.W, K.H, True, True)
        m = BR.mosaic(fr, dp)
        upload = synth.raw_frame(m, 16, RAW12["valid_bit"], True, True, np.random.default_rng(3))
        assert np.array_equal(RR.T(upload, RAW12["valid_bit"], True, True), m)
        images = [BR.demosaic(m[f], dp) for f in range(N)]
    elif variant == "enh":
        upload = ER.dim(fr, 80)
        images = [ER.E(f, 100.0, 50.0)[0] for f in upload]
        assert any(not np.array_equal(images[f], upload[f]) for f in range(N))
    elif variant == "win":
        upload = fr
        images = [np.ascontiguousarray(fr[f][y:y + K.WIN_H, x:x + K.WIN_W]) for f, (x, y) in enumerate(K.WIN_ORIGINS)]
    else:
        upload, images = fr, list(fr)
    cases = K.icon_cases(*size)
    per_frame = [armours_of([q for _, q in cases[s]]) for s in K.split(len(cases), N)]
    assert len({len(a) for a in per_frame}) >= 3 and all(9 <= len(a) <= CAP for a in per_frame)
    return dict(upload=upload, images=images, size=size, armours=per_frame, names=[[n for n, _ in cases[s]] for s in K.split(len(cases), N)])


@functools.lru_cache(maxsize=None)
def reference(variant, model_names=None):
    """[(identities, armours after the clamp, icons)] per frame from the oracle; model_names: one vote case per frame, else MODEL"""
    import oracle_lib as O
    O.set_math_mode(0)
    m = material(variant)
    return [O.classify_armours(m["images"][f], m["armours"][f], MODEL if model_names is None else K.model_of(BY_NAME[model_names[f]])) for f in range(N)]


@pytest.fixture(scope="module")
def ctxs():
    """one context per variant, made on first use and closed with the module"""
    made = {}

    def get(variant):
        if variant not in made:
            c = Context(device=0, max_frames=N, max_width=K.W, max_height=K.H, max_armours=CAP)
            if variant in BAYER8:
                c.set_input_format(BAYER8[variant])
            if variant == "raw12":
                c.set_input_format(RAW12["pattern"])
                c.set_input_layout(RAW12["bits"], RAW12["valid_bit"], RAW12["mirror"], RAW12["flip"])
            if variant == "enh":
                c.set_enhance(True)
            made[variant] = c
        return made[variant]
    yield get
    for c in made.values():
        c.close()


def up(dst, src):
    assert lib().rmcv_device_upload(0, C.c_void_p(dst), ptr(src), C.c_int64(src.nbytes)) == 0


def bind_and_inject(c, variant):
    """the variant's frames bound and run through a pixel pass that finds nothing, then every frame's case armours put into the batch's table"""
    m = material(variant)
    c.upload(m["upload"])
    if variant == "win":
        c.set_windows(np.array(K.WIN_ORIGINS, np.int32), K.WIN_W, K.WIN_H)
        assert np.array_equal(c.windows()[0], np.array(K.WIN_ORIGINS, np.int32))
    c.run(default_params(**QUIET), STAGE_ALL)
    c.sync()
    k = c.counts()
    assert not k["n_armours"].any() and not k["status"].any()
    d_arm, d_cnt, cap, n = c.device_views()
    assert cap == CAP and n == N
    table, counts = np.zeros((N, CAP), abi.ARMOUR), np.zeros(N, np.int32)
    for f, a in enumerate(m["armours"]):
        table[f, :len(a)], counts[f] = a, len(a)
    up(d_arm, table)
    up(d_cnt, counts)
    return m, table


def check_batch(c, m, ref):
    c.sync()
    arm, offs = c.armours()
    ident = c.identities()
    assert offs.tolist() == np.concatenate([[0], np.cumsum([len(a) for a in m["armours"]])]).tolist()
    for f, (ri, ra, ricons) in enumerate(ref):
        got = arm[offs[f]:offs[f + 1]]
        bad = [m["names"][f][i] for i in range(len(ra)) if got[i].tobytes() != ra[i].tobytes()]
        assert not bad, (f, "armour table", bad)
        icons = c.icons(f)
        bad = [m["names"][f][i] for i in range(len(ra)) if not np.array_equal(icons[i], ricons[i])]
        assert not bad, (f, "icons", bad)
        bad = [m["names"][f][i] for i in range(len(ra)) if ident[offs[f] + i] != ri[i]]
        assert not bad, (f, "identities", bad)


# ---------------------------------------------------------------- 1. rmcv_classify_armours
@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "win"])
def test_classify_armours_every_case(ctxs, variant):
    c, m = ctxs(variant), material(variant)
    c.svm_load(*MODEL)
    seen = set()
    for f, (ri, ra, ricons) in enumerate(reference(variant)):
        gi, ga, gicons = c.classify_armours(m["upload"][f], m["armours"][f])
        bad = [m["names"][f][i] for i in range(len(ra)) if ga[i].tobytes() != ra[i].tobytes()]
        assert not bad, (f, "armour table", bad)
        bad = [m["names"][f][i] for i in range(len(ra)) if not np.array_equal(gicons[i], ricons[i])]
        assert not bad, (f, "icons", bad)
        assert np.array_equal(gi, ri), f
        seen |= set(ri.tolist())
    assert len(seen) >= 3                                                     # the model tells the icons apart


# ---------------------------------------------------------------- 2. the batch classifier on injected armours
@pytest.mark.parametrize("variant", ["bgr", "win", "bg", "raw12", "enh"])
def test_batch_classifier_on_injected_armours(ctxs, variant):
    c = ctxs(variant)
    c.svm_load(*MODEL)
    try:
        m, _ = bind_and_inject(c, variant)
        c.run(default_params(**QUIET), STAGE_IDENTITY)                        # alone: k_classify*, not the fused tail
        check_batch(c, m, reference(variant))
    finally:
        if variant == "win":
            c.set_windows(None, 0, 0)


# ---------------------------------------------------------------- 3. a model table and per-frame indices
@pytest.mark.parametrize("variant", ["bgr", "win", "bg", "enh"])
def test_model_table_on_injected_armours(ctxs, variant):
    c = ctxs(variant)
    c.svm_load_models([K.model_of(BY_NAME[t]) for t in TABLE])
    assert len({BY_NAME[t][4] for t in TABLE}) >= 4                           # models of different n_class
    try:
        m, _ = bind_and_inject(c, variant)
        c.set_frame_models(MODEL_IDX)
        c.run(default_params(**QUIET), STAGE_IDENTITY)
        check_batch(c, m, reference(variant, tuple(TABLE[i] for i in MODEL_IDX)))
        assert np.array_equal(c.frame_models(), MODEL_IDX)
    finally:                                                                  # the context is shared: leave it as the next test expects it
        c.set_frame_models(None)
        if variant == "win":
            c.set_windows(None, 0, 0)
        c.svm_load(*MODEL)


# ---------------------------------------------------------------- 4. the harvest and the novelty append
@pytest.mark.parametrize("variant", ["bgr", "gr", "enh"])
def test_harvest_rows_and_novelty(ctxs, variant):
    c = ctxs(variant)
    m, table = bind_and_inject(c, variant)
    ref = reference(variant)
    rows = np.concatenate([r[2].reshape(len(r[2]), -1) for r in ref])
    quads = np.concatenate([r[1]["icon"] for r in ref])
    n_rows = [len(a) for a in m["armours"]]
    labels = np.arange(N, dtype=np.int32) + 1
    ds = DeviceDataset(c, 512)
    c.harvest(ds, labels, tag=4)
    assert (ds.count, ds.dropped) == (len(rows), 0)
    got, meta = ds.rows(), ds.meta()
    names = [n for f in range(N) for n in m["names"][f]]
    bad = [names[i] for i in range(len(rows)) if not np.array_equal(got[i], rows[i])]
    assert not bad, bad
    bad = [names[i] for i in range(len(rows)) if meta["icon"][i].tobytes() != quads[i].tobytes()]
    assert not bad, bad
    assert np.array_equal(meta["frame"], np.repeat(np.arange(N), n_rows)) and np.array_equal(meta["label"], np.repeat(labels, n_rows))
    arm, offs = c.armours()
    assert all(arm[offs[f]:offs[f + 1]].tobytes() == table[f, :n_rows[f]].tobytes() for f in range(N))     # the table is only read: still unclamped
    ds.close()
    # the novelty append: the same rows through the rings' rule
    R_, T = 4, 20000
    state = NR.State(N, R_)
    keep, _, _ = NR.append(state, T, rows, n_rows, labels)
    assert keep.any() and not keep.all()
    ds = DeviceDataset(c, 512)
    ds.set_novelty(R_, T)
    c.harvest(ds, labels, tag=5)
    assert ds.count == int(keep.sum()) and ds.novelty["near"] == state.near
    got, meta = ds.rows(), ds.meta()
    assert np.array_equal(got, rows[keep]) and meta["icon"].tobytes() == quads[keep].tobytes()
    rings, pushed = ds.rings()
    assert np.array_equal(pushed, state.pushed) and np.array_equal(rings, state.rings)
    ds.close()


# ---------------------------------------------------------------- 5. the vote cases
def test_vote_cases_through_svm_predict_and_the_dataset(ctxs):
    c = ctxs("bgr")
    cases = K.vote_cases()
    rows = np.stack([K.rows_from(K.frame(), [dict(K.named_icons(K.W, K.H))[k]])[0] for k in K.ROW_SOURCES])
    ds = DeviceDataset(c, 8)
    d_rows, d_meta, d_count = ds.device()
    up(d_rows, np.ascontiguousarray(rows))
    up(d_count, np.array([len(rows)], np.int32))
    try:
        for name, wts, rho, labels, n_class, row, src in cases:
            want = K.vote(wts, rho, labels, n_class, row)[0]
            assert np.array_equal(row, rows[src])
            c.svm_load(wts, rho, labels)
            assert c.svm_predict(row[None])[0] == want, name
            assert ds.predict([src])[0] == want, name
        # ... and as entries of a model table.  The table refuses a rho that is not finite (rmcv_svm_load_models), so the cases with a NaN
        # rho cannot go into one: they went through svm_load above.  Every other case does, MAX_MODELS entries to a table.
        able = [t for t in BY_NAME if finite(t)]
        assert len(able) + sum(bool(np.isnan(c_[2]).any()) for c_ in cases) == len(cases) and len(able) > MR.MAX_MODELS
        done = []
        for first in range(0, len(able), MR.MAX_MODELS):
            table = able[first:first + MR.MAX_MODELS]
            c.svm_load_models([K.model_of(BY_NAME[t]) for t in table])
            for k, t in enumerate(table):
                name, wts, rho, labels, n_class, row, src = BY_NAME[t]
                assert c.svm_predict(row[None], model=k)[0] == K.vote(wts, rho, labels, n_class, row)[0], t
                done.append(t)
        assert len(done) == len(able) and set(done) == set(able)
    finally:
        c.svm_load(*MODEL)
        ds.close()


@pytest.mark.parametrize("variant", ["bgr", "bg", "enh"])
def test_vote_cases_through_the_classifier_kernels(ctxs, variant):
    """the row of a vote case is the icon of one named case on frame 0: that icon classified under the case's model gives the case's label.
    BGR sees frame 0 itself, so the list's own rows and last-bit cases apply.  Bayer and the gamma table cut other rows from D(m) and E(f):
    the cases whose weights are zero apply to any row, and the last-bit cases are built anew on the row the oracle cuts there (K.edge_cases)"""
    import oracle_lib as O
    c, m = ctxs(variant), material(variant)
    named = dict(K.named_icons(K.W, K.H))
    arm = armours_of([named[k] for k in K.ROW_SOURCES])
    _, _, icons = O.classify_armours(m["images"][0], arm, MODEL)
    mine = [icons[src].reshape(-1) for src in range(len(arm))]
    if variant == "bgr":
        todo = [(name, wts, rho, labels, n_class, src) for name, wts, rho, labels, n_class, row, src in K.vote_cases()]
        assert all(np.array_equal(mine[src], row) for _, _, _, _, _, row, src in K.vote_cases())
    else:
        todo = [(name, wts, rho, labels, n_class, src) for name, wts, rho, labels, n_class, row, src in K.vote_cases() if not name.startswith("edge_")]
        assert not any(np.array_equal(mine[src], BY_NAME["edge_%d_2_at" % src][5]) for src in range(len(arm)))     # other rows indeed
        for src in range(len(arm)):
            todo += [(name, wts, rho, labels, n_class, src) for name, wts, rho, labels, n_class in K.edge_cases(mine[src], 77 + src, "edge_%s_%d" % (variant, src))]
    assert sum(name.startswith("edge_") for name, *_ in todo) == 12 * len(arm)
    try:
        for name, wts, rho, labels, n_class, src in todo:
            c.svm_load(wts, rho, labels)
            gi, _, gicons = c.classify_armours(m["upload"][0], arm[src:src + 1])
            assert np.array_equal(gicons[0].reshape(-1), mine[src]) and gi[0] == K.vote(wts, rho, labels, n_class, mine[src])[0], name
    finally:
        c.svm_load(*MODEL)


# ---------------------------------------------------------------- 6. the fused tail
def test_fused_tail_clamps_on_all_four_sides(oracle):
    img = K.tail_scene()
    c = Context(device=0, max_frames=3, max_width=K.TAIL_W, max_height=K.TAIL_H)
    try:
        c.svm_load(*MODEL)
        batch = np.stack([img, img[::-1, ::-1], img])                         # (the scene turned by 180 degrees too: other corners, other edges)
        c.upload(batch)
        c.run(default_params(), STAGE_ALL | STAGE_IDENTITY)                   # BGR, no windows, no table: the sparse kernel's own classifier
        c.sync()
        arm, offs = c.armours()
        ident = c.identities()
        for f in range(3):
            found = oracle.detect_frame(np.ascontiguousarray(batch[f]))["armours"]
            ri, ra, ricons = oracle.classify_armours(np.ascontiguousarray(batch[f]), found, MODEL)
            assert len(found) == len(K.TAIL_PAIRS)
            assert arm[offs[f]:offs[f + 1]].tobytes() == ra.tobytes(), f
            assert np.array_equal(c.icons(f), ricons) and np.array_equal(ident[offs[f]:offs[f + 1]], ri), f
            assert K.sides_clamped(found["icon"], arm[offs[f]:offs[f + 1]]["icon"], K.TAIL_W, K.TAIL_H) == (True, True, True, True), f
    finally:
        c.close()
