"""Per-stream icon models on the GPU: the context's model table selected per frame by k_classify_models
(rmcv_svm_load_models, rmcv_batch_set_[device_]frame_models, rmcv_pipeline_set_frame_models, rmcv_svm_predict_model).  Identities, icons
and clamped icon vertices are held, byte for byte, against oracle.classify_armours with each frame's model, and -- for the three readers
of the frames -- against the same context run once per model through rmcv_svm_load, the single-model kernels.  Nothing has a tolerance;
every GPU step runs once.

The scene is synth.batch(900, 12, 320, 256): frames 900 .. 910 hold 2, 5, 11, 8, 2, 2, 2, 9, 13, 4, 6 armours, frame 911 none.  The four
models give four different identity vectors on every frame with armours, and the 8-class model returns label 7 on frame 902."""
import ctypes as C

import numpy as np
import pytest

import bayer_ref as BR
import enhance_ref as ER
import raw_ref as RR
from rmcv_amd import (BAYER_GB, BAYER_RG, CAMP_BLUE, HARVEST_MISSES, STAGE_ALL, STAGE_IDENTITY, Context, DeviceDataset, Pipeline, RmcvError, abi,
                      default_params, harvest_plan, svm, synth)
from test_gpu_attitude import device_array, download
from test_gpu_window import first_armour_origins

pytestmark = pytest.mark.gpu

N, W, H = 12, 320, 256
COUNTS = [2, 5, 11, 8, 2, 2, 2, 9, 13, 4, 6, 0]
IDX = [1, 2, 3, 0, 1, 2, 3, 0, 3, 2, 1, 0]
C5 = STAGE_ALL | STAGE_IDENTITY


def the_models():
    w3, r3, _ = synth.svm_weights(11, 3)
    return [synth.svm_weights(20241008, 7), synth.svm_weights(7, 7), (w3, r3, np.array([40, 41, 42], np.int32)), synth.svm_weights(13, 8)]


@pytest.fixture(scope="module")
def scene(oracle):
    """frames, models, and want[k][f] = (identities, armours, icons) of frame f under model k on the CPU oracle, computed once"""
    frames = synth.batch(900, N, W, H, CAMP_BLUE, 0)
    models = the_models()
    arms = [oracle.detect_frame(f, oracle.default_params())["armours"] for f in frames]
    assert [len(a) for a in arms] == COUNTS
    want = [[oracle.classify_armours(frames[f], arms[f], m) for f in range(N)] for m in models]
    for f in range(N - 1):
        assert len({want[k][f][0].tobytes() for k in range(4)}) == 4, f          # the four models tell on every frame with armours
    assert 7 in want[3][2][0]                                                   # a label only the 8-class model has
    return frames, models, want


def results(c, n=N):
    """per frame of the context's batch (run and synced): (armour bytes, identity bytes, icon bytes)"""
    arm, offs = c.armours()
    ident = c.identities()
    return [(arm[offs[f]:offs[f + 1]].tobytes(), ident[offs[f]:offs[f + 1]].tobytes(), c.icons(f).tobytes()) for f in range(n)]


def wanted(want, idx):
    return [(want[k][f][1].tobytes(), want[k][f][0].tobytes(), want[k][f][2].tobytes()) for f, k in enumerate(idx)]


def run(c, stages=C5):
    c.run(default_params(), stages)
    c.sync()


def table_context(scene, **limits):
    frames, models, _ = scene
    c = Context(device=0, max_frames=N, max_width=W, max_height=H, **limits)
    c.svm_load_models(models)
    c.upload(frames)
    return c


# ---------------------------------------------------------------- 1. the table against the oracle
def test_table_against_the_oracle(scene):
    frames, models, want = scene
    c = table_context(scene)
    assert c.frame_models().tolist() == [0] * N                             # selection is off until it is set
    c.set_frame_models(IDX)
    run(c)
    assert results(c) == wanted(want, IDX)
    assert c.frame_models().tolist() == IDX
    # selection off: every frame through model 0
    c.set_frame_models(None)
    run(c)
    assert results(c) == wanted(want, [0] * N) and c.frame_models().tolist() == [0] * N
    # a new binding returns to off
    c.set_frame_models(IDX)
    c.upload(frames)
    run(c)
    assert results(c) == wanted(want, [0] * N) and c.frame_models().tolist() == [0] * N
    # rmcv_svm_load afterwards: a table of one, selection off
    c.set_frame_models(IDX)
    c.svm_load(*models[1])
    run(c)
    assert results(c) == wanted(want, [1] * N) and c.frame_models().tolist() == [0] * N
    with pytest.raises(RmcvError) as e:
        c.set_frame_models([0] * (N - 1) + [1])                             # ... of ONE
    assert e.value.code == abi.ERR_BAD_ARG and "frame 11: model 1 is outside the table (0 .. 0)" in str(e.value)
    # the single-model entry points use entry 0 whatever the frames' models are
    c.svm_load_models(models[::-1])                                         # entry 0: the 8-class model
    arms2 = np.frombuffer(want[0][2][1].tobytes(), abi.ARMOUR)
    gi, ga, gicons = c.classify_armours(frames[2], arms2)
    assert (ga.tobytes(), gi.tobytes(), gicons.tobytes()) == wanted(want, [0, 0, 3])[2]
    rows = want[0][2][2].reshape(COUNTS[2], abi.SVM_FEATURES)               # the icons of frame 902
    assert c.svm_predict(rows).tolist() == svm.Model(*models[3]).predict(rows).tolist() == want[3][2][0].tolist()
    for k in range(4):                                                      # rmcv_svm_predict_model against rmcv_svm_predict_host with entry k
        assert c.svm_predict(rows, model=k).tolist() == svm.Model(*models[3 - k]).predict(rows).tolist() == want[3 - k][2][0].tolist(), k
    with pytest.raises(RmcvError) as e:
        c.svm_predict(rows, model=4)
    assert e.value.code == abi.ERR_BAD_ARG and "model 4 is outside the table (0 .. 3)" in str(e.value)
    # what a table refuses, before any GPU work: the table loaded stays
    bad = list(models)
    bad[2] = (models[2][0].copy(), models[2][1].copy(), models[2][2])
    bad[2][1][1] = np.nan
    for arg, what in ((bad, "model 2: rho 1 is not finite"), (models * 17, "n_models 68 is out of range (1 .. 64)")):
        with pytest.raises(RmcvError) as e:
            c.svm_load_models(arg)
        assert e.value.code == abi.ERR_BAD_ARG and what in str(e.value), str(e.value)
    assert c.svm_predict(rows, model=3).tolist() == want[0][2][0].tolist()
    assert c.check_guards()[0] == 0
    c.close()


# ---------------------------------------------------------------- 2. raw indices from the device
def test_raw_indices_from_the_device(scene):
    frames, models, want = scene
    stray = [-1, 4, 2**31 - 1, -2**31, 1, 2, 3, 0, 64, 3, 1, 5]
    eff = [0, 0, 0, 0, 1, 2, 3, 0, 0, 3, 1, 0]
    assert [abi.frame_model(i, 4) for i in stray] == eff
    c = table_context(scene)
    # the host setter refuses the list, and the table it had stays in force
    c.set_frame_models(IDX)
    with pytest.raises(RmcvError) as e:
        c.set_frame_models(stray)
    assert e.value.code == abi.ERR_BAD_ARG and "frame 0: model -1 is outside the table (0 .. 3)" in str(e.value)
    with pytest.raises(RmcvError) as e:
        c.set_frame_models([0, 4] + [0] * (N - 2))
    assert e.value.code == abi.ERR_BAD_ARG and "frame 1: model 4" in str(e.value)
    # in device memory any value may stand: the rule makes it an entry of the table
    d = device_array(np.array(stray, np.int32))
    c.set_frame_models(d.data_ptr(), keepalive=d)
    run(c)
    assert results(c) == wanted(want, eff) and c.frame_models().tolist() == eff
    # borrowed: rewritten on the device, the next run follows it without a new binding
    import torch
    d.copy_(torch.from_numpy(np.array(IDX, np.int32)))
    torch.cuda.synchronize()
    run(c)
    assert results(c) == wanted(want, IDX) and c.frame_models().tolist() == IDX
    assert c.check_guards()[0] == 0
    c.close()


# ---------------------------------------------------------------- 3. capacity
def test_capacity_of_four_armours(scene, oracle):
    frames, models, _ = scene
    c = table_context(scene, max_armours=4)

    def tables():
        """identities [frame][4] and the icons per frame, read without the armour list (frames beyond the limit refuse that)"""
        n = c.counts()["n_armours"]
        ident = c.identities()
        at = np.concatenate([[0], np.cumsum(n)])
        return n, [ident[at[f]:at[f + 1]].tobytes() for f in range(N)], [c.icons(f) for f in range(N)]

    c.set_frame_models(IDX)
    run(c)
    n, ident, icons = tables()
    assert n.tolist() == [min(k, 4) for k in COUNTS]
    d_arm = c.device_views()[0]
    arm = download(d_arm, abi.ARMOUR, N * 4).reshape(N, 4)
    ri, ra, ricons = oracle.classify_armours(frames[8], arm[8], models[IDX[8]])   # frame 908: its first 4 armours, the 8-class model
    assert ident[8] == ri.tobytes() and icons[8].tobytes() == ricons.tobytes() and ra.tobytes() == arm[8].tobytes()
    for f in range(N):                                                      # ... and every other frame its own rows with its own model
        ri, ra, ricons = oracle.classify_armours(frames[f], arm[f, :n[f]], models[IDX[f]])
        assert ident[f] == ri.tobytes() and icons[f].tobytes() == ricons.tobytes(), f
    # frame 908 replaced by the empty frame: its neighbours' rows do not move
    other = frames.copy()
    other[8] = frames[11]
    c.upload(other)
    c.set_frame_models(IDX)
    run(c)
    n2, ident2, icons2 = tables()
    assert n2[8] == 0 and n2.tolist()[:8] + n2.tolist()[9:] == n.tolist()[:8] + n.tolist()[9:]
    for f in (7, 9):
        assert ident2[f] == ident[f] and icons2[f].tobytes() == icons[f].tobytes(), f
    assert c.check_guards()[0] == 0                                         # nothing outside [f][0 .. 3]
    c.close()


# ---------------------------------------------------------------- 4. the three readers of the frames
def reader_variants(oracle, frames6):
    """(name, configure(context), what to upload, windows or None)"""
    origins, _ = first_armour_origins(oracle, frames6, 160, 128)
    dp = RR.derived_pattern(BAYER_GB, W, H, True, False)
    raw = synth.raw_frame(BR.mosaic(frames6, dp), 16, 4, True, False, np.random.default_rng(5))

    def layout(c):
        c.set_input_format(BAYER_GB)
        c.set_input_layout(16, 4, True, False)
    return [("windows", lambda c: None, frames6, (origins, 160, 128)),
            ("bayer RG 8-bit", lambda c: c.set_input_format(BAYER_RG), synth.mosaic(frames6, BAYER_RG), None),
            ("16-bit, valid bit 4, mirrored", layout, raw, None),
            ("enhance", lambda c: c.set_enhance(True), ER.dim(frames6, 80), None)]


@pytest.mark.parametrize("which", range(4), ids=["windows", "bayer", "layout", "enhance"])
def test_the_three_readers(scene, oracle, which):
    frames, models, _ = scene
    name, configure, data, win = reader_variants(oracle, frames[:6])[which]
    idx = IDX[:6]
    c = Context(device=0, max_frames=6, max_width=W, max_height=H)
    configure(c)

    def bind():
        c.upload(data)
        if win:
            c.set_windows(*win)

    # the same context, once per model through rmcv_svm_load: the single-model kernels
    single = []
    for k in range(4):
        c.svm_load(*models[k])
        bind()
        run(c)
        single.append(results(c, 6))
    c.svm_load_models(models)
    bind()
    c.set_frame_models(idx)
    run(c)
    got = results(c, 6)
    assert got == [single[idx[f]][f] for f in range(6)], name
    assert c.frame_models().tolist() == idx
    used = {idx[f] for f in range(6) if got[f][1]}
    assert len(used) >= 2, (name, used)                                     # armours under at least two different models
    assert any(single[0][f][1] != got[f][1] for f in range(6)), name       # ... and the models tell
    assert c.check_guards()[0] == 0
    c.close()


# ---------------------------------------------------------------- 5. pipeline
def test_pipeline_sticky_index_table(scene):
    frames, models, want = scene
    other = [3, 3, 0, 1, 2, 0, 1, 2, 3, 0, 2, 1]
    pl = Pipeline(device=0, depth=2, max_frames=N, max_width=W, max_height=H)
    for cc in pl.contexts:
        cc.svm_load_models(models)
    dev = device_array(frames)
    d_idx, d_other = device_array(np.array(IDX, np.int32)), device_array(np.array(other, np.int32))
    p = default_params()

    def got(t, idx):
        pl.wait(t)
        cc = pl.context_of(t)
        assert cc.frame_models().tolist() == idx
        return results(cc)

    # no table set: model 0 for every frame
    t = pl.submit(dev.data_ptr(), N, H, W, p, C5)
    assert got(t, [0] * N) == wanted(want, [0] * N)
    pl.set_frame_models(d_idx.data_ptr(), N, keepalive=(d_idx, d_other))    # once: it sticks
    t0 = pl.submit(dev.data_ptr(), N, H, W, p, C5)
    t1 = pl.submit(dev.data_ptr(), N, H, W, p, C5)
    assert got(t0, IDX) == wanted(want, IDX) and got(t1, IDX) == wanted(want, IDX)
    import torch
    d_idx.copy_(d_other)                                                    # swapped on the device between submits 2 and 3
    torch.cuda.synchronize()
    t2 = pl.submit(dev.data_ptr(), N, H, W, p, C5)
    assert got(t2, other) == wanted(want, other)
    assert pl.get_info().host_blocking_calls == 0

    def refused(what, n_frames):
        before = pl.get_info().submitted
        with pytest.raises(RmcvError) as e:
            pl.submit(dev.data_ptr(), n_frames, H, W, p, C5)
        assert e.value.code == abi.ERR_BAD_ARG and what in str(e.value), str(e.value)
        assert pl.get_info().submitted == before

    # a submit with the classifier whose n_frames is not the table's (one without it does not read the table: accepted)
    refused("model index table 12", N - 1)
    pl.wait(pl.submit(dev.data_ptr(), N - 1, H, W, p, STAGE_ALL))
    # slots holding 4 and 3 models
    pl.drain()
    pl.contexts[1].svm_load_models(models[:3])
    refused("n_models differs", N)
    pl.contexts[1].svm_load_models(models)
    t = pl.submit(dev.data_ptr(), N, H, W, p, C5)
    assert got(t, other) == wanted(want, other)
    # off again
    pl.set_frame_models(None)
    t = pl.submit(dev.data_ptr(), N, H, W, p, C5)
    assert got(t, [0] * N) == wanted(want, [0] * N)
    assert pl.get_info().host_blocking_calls == 0
    assert all(cc.check_guards()[0] == 0 for cc in pl.contexts)
    pl.close()


# ---------------------------------------------------------------- 6. camps as indices: main.cpp:21-22 for a mixed fleet
def test_camps_as_model_indices(scene):
    frames, models, want = scene
    n, camps, eff = 6, [0, 1, 1, 0, 2, -1], [0, 1, 1, 0, 0, 0]
    pair = models[:2]                                                       # {svm_red, svm_blue}
    # per frame: a single-model run of the whole batch with that frame's camp and that camp's model
    c = Context(device=0, max_frames=n, max_width=W, max_height=H)
    single = {}
    for camp, k in sorted(set(zip(camps, eff))):
        c.svm_load(*pair[k])
        c.upload(frames[:n])
        c.run(default_params(camp=camp), C5)
        c.sync()
        single[camp] = results(c, n)
    c.close()
    pl = Pipeline(device=0, depth=2, max_frames=n, max_width=W, max_height=H)
    for cc in pl.contexts:
        cc.svm_load_models(pair)
    dev = device_array(frames[:n])
    d_camps = device_array(np.array(camps, np.int32))
    pl.set_frame_models(d_camps.data_ptr(), n, keepalive=d_camps)           # the camps table as it is
    t = pl.submit(dev.data_ptr(), n, H, W, default_params(), C5, camps=(d_camps.data_ptr(), None))
    pl.wait(t)
    cc = pl.context_of(t)
    assert cc.frame_models().tolist() == eff
    got = results(cc, n)
    assert got == [single[camps[f]][f] for f in range(n)]
    # the blue streams' frames (the scene's enemy colour) are svm_blue's on the oracle, and svm_red would have said otherwise
    for f in (1, 2):
        assert got[f] == wanted(want, [1] * n)[f] and got[f][1] != want[0][f][0].tobytes(), f
    assert pl.get_info().host_blocking_calls == 0
    pl.close()


# ---------------------------------------------------------------- 7. the harvest keeps what each stream's OWN model gets wrong
def test_harvest_misses_under_selection(scene):
    frames, models, want = scene
    c = table_context(scene)
    c.set_frame_models(IDX)
    run(c)
    arm, offs = c.armours()
    k = c.counts()
    cap = c.limits.max_armours
    ident = np.full((N, cap), -7, np.int32)
    for f in range(N):
        ident[f, :COUNTS[f]] = want[IDX[f]][f][0]                           # the identities of test 1
    labels = np.array([want[IDX[f]][f][0][0] if COUNTS[f] and f % 2 == 0 else 99 for f in range(N)], np.int32)
    ds = DeviceDataset(c, 128)
    c.harvest(ds, labels, HARVEST_MISSES, tag=3)
    items, count, _ = harvest_plan(k["n_armours"], k["status"], labels, ident, cap, HARVEST_MISSES, 0, 128)
    assert 0 < count < len(arm) and ds.count == count                       # both kinds occur
    rows = np.array([want[IDX[f]][f][2][a].reshape(-1) for f, a, _ in items], np.uint8)
    assert np.array_equal(ds.rows(0, count), rows)
    assert all(ident[f][a] != labels[f] for f, a, _ in items)
    ds.close()
    c.close()
