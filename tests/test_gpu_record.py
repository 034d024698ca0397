"""The session recorder on the GPU.  rmcv_pack_frames writes the bytes of the specification's numpy restatement
(tests/pack_ref.py) and rmcv_unpack_frames gives the input back, on every shape, lag and kind of input of the case list; a pipeline with a
recorder keeps the chosen frames of its last batches bit for bit, with ticket, geometry, parameters, user blob, frame keys and window
origins, without a blocking call in submit and without changing a single armour; a saved session replays to the same armours."""
import ctypes as C

import numpy as np
import pytest

import pack_ref as R
from rmcv_amd import BAYER_RG, CAMP_BLUE, STAGE_ALL, Pipeline, Recorder, Session, abi, default_params, pack_bound, synth
from rmcv_amd.abi import RmcvError, lib, ptr

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. the packing kernels against the restatement
class DevBuf:
    """device memory through the ABI's own helpers (synchronous copies on the library's runtime)"""

    def __init__(self, nbytes):
        self.p, self.n = C.c_void_p(), int(nbytes)
        assert lib().rmcv_device_alloc(0, C.c_int64(self.n), C.byref(self.p)) == 0

    def put(self, a):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.n and lib().rmcv_device_upload(0, self.p, ptr(a), C.c_int64(a.nbytes)) == 0

    def get(self, nbytes, dtype=np.uint8):
        out = np.empty(int(nbytes) // np.dtype(dtype).itemsize, dtype)
        assert lib().rmcv_device_download(0, ptr(out), self.p, C.c_int64(out.nbytes)) == 0
        return out

    def free(self):
        lib().rmcv_device_free(0, self.p)


@pytest.fixture(scope="module")
def bufs():
    w, h = max(R.WIDTHS), max(R.HEIGHTS)
    frame_bytes = 3 * ((w + 5) * h + 11)
    b = {"in": DevBuf(frame_bytes), "out": DevBuf(3 * (pack_bound(w, h) + 64)), "sizes": DevBuf(3 * 8), "back": DevBuf(frame_bytes)}
    yield b
    for v in b.values():
        v.free()


GROUPS = [(k,) for k in R.KINDS] + [R.KINDS[:3], R.KINDS[3:]]       # n = 1 for every kind, n = 3 twice


@pytest.mark.parametrize("w", R.WIDTHS)
def test_pack_frames_equals_the_restatement_and_unpack_frames_inverts_it(bufs, w):
    L = lib()
    for h in R.HEIGHTS:
        stride, bound = w + 5, pack_bound(w, h)
        pitch, out_pitch = stride * h + 11, R.align8(bound + 24)     # a frame pitch larger than the frame; areas larger than the bound
        for lag in (1, 2, 3, 4):
            for kinds in GROUPS:
                n = len(kinds)
                host = np.full((n, pitch), 0xEE, np.uint8)
                for f, kind in enumerate(kinds):
                    host[f, :stride * h].reshape(h, stride)[:, :w] = R.plane(kind, w, h)
                bufs["in"].put(host)
                bufs["out"].put(np.full(n * out_pitch, 0xCD, np.uint8))
                rc = L.rmcv_pack_frames(0, bufs["in"].p, n, w, h, stride, C.c_int64(pitch), lag, bufs["out"].p, C.c_int64(out_pitch), bufs["sizes"].p, None)
                assert rc == 0
                sizes = bufs["sizes"].get(8 * n, np.int64)
                got = bufs["out"].get(n * out_pitch).reshape(n, out_pitch)
                for f, kind in enumerate(kinds):
                    want = R.packed(kind, w, h, lag)
                    assert sizes[f] == len(want), (kind, w, h, lag, n)
                    assert got[f, :len(want)].tobytes() == want.tobytes(), (kind, w, h, lag, n)
                    assert (got[f, bound:] == 0xCD).all()                                   # nothing beyond the bound
                bufs["back"].put(np.full((n, pitch), 0x77, np.uint8))
                rc = L.rmcv_unpack_frames(0, bufs["out"].p, n, w, h, C.c_int64(out_pitch), lag, bufs["back"].p, stride, C.c_int64(pitch), None)
                assert rc == 0
                back = bufs["back"].get(n * pitch).reshape(n, pitch)
                for f in range(n):
                    rows = back[f, :stride * h].reshape(h, stride)
                    assert np.array_equal(rows[:, :w], host[f, :stride * h].reshape(h, stride)[:, :w]), (kinds[f], w, h, lag, n)
                    assert (rows[:, w:] == 0x77).all() and (back[f, stride * h:] == 0x77).all()  # bytes beyond w_bytes untouched


def test_pack_frames_refuses_bad_arguments(bufs):
    L = lib()
    ok = [0, bufs["in"].p, 1, 300, 4, 300, C.c_int64(1200), 3, bufs["out"].p, C.c_int64(R.align8(pack_bound(300, 4))), bufs["sizes"].p, None]
    assert L.rmcv_pack_frames(*ok) == 0
    for at, bad in ((1, None), (2, 0), (3, 0), (4, 0), (5, 299), (7, 0), (7, 5), (8, None), (9, C.c_int64(pack_bound(300, 4) - 8)), (9, C.c_int64(pack_bound(300, 4) + 4)),
                    (10, None)):
        args = list(ok)
        args[at] = bad
        assert L.rmcv_pack_frames(*args) == abi.ERR_BAD_ARG, at


# ---------------------------------------------------------------- 2. a pipeline's recorder
W, H, N = 160, 96, 4
CHOSEN = [0, 3]
FIRST = (3, 6, 18)        # synth streams whose frames 0 and 3 at 160 x 96 hold an armour each (checked against the oracle below)


def make_pipeline(**kw):
    return Pipeline(device=0, depth=2, max_frames=N, max_width=W, max_height=H, **kw)


def run_three(pl, dev, params, **kw):
    """three batches through a depth-2 pipeline -> [(armours, offs)] per ticket"""
    out, tickets = [], []
    for i in range(3):
        tickets.append(pl.submit(dev[i].data_ptr(), N, H, W, params[i], STAGE_ALL, **kw))
        if i >= 1:
            out.append(pl.collect(tickets[i - 1]))
    out.append(pl.collect(tickets[2]))
    assert tickets == [0, 1, 2]
    return out


@pytest.fixture(scope="module")
def batches():
    import torch
    host = [synth.batch(f, N, W, H, CAMP_BLUE, 0, threads=2) for f in FIRST]
    return host, [torch.from_numpy(b).cuda() for b in host]


@pytest.fixture(scope="module")
def recorded(batches, tmp_path_factory):
    """the reference run: three batches with a recorder of two slots on frames [0, 3]; the session saved from it"""
    host, dev = batches
    params = [default_params(lower_bound=80 - i) for i in range(3)]
    plain = make_pipeline()
    want = run_three(plain, dev, params)
    plain.close()
    rec = Recorder(device=0, slots=2, max_frames=2, max_w_bytes=3 * W, max_h=H, user_bytes=64)
    pl = make_pipeline()
    pl.set_recorder(rec, CHOSEN)
    got, tickets = [], []
    for i in range(3):
        rec.set_user(b"batch %d" % i)
        tickets.append(pl.submit(dev[i].data_ptr(), N, H, W, params[i], STAGE_ALL))
        if i >= 1:
            got.append(pl.collect(tickets[i - 1]))
    got.append(pl.collect(tickets[2]))
    path = str(tmp_path_factory.mktemp("session") / "three.rmcv")
    rec.save(path)
    yield {"pl": pl, "rec": rec, "want": want, "got": got, "params": params, "path": path}
    pl.close()
    rec.close()


def test_recorder_holds_the_last_batches_bit_for_bit(batches, recorded):
    host, _ = batches
    rec, pl = recorded["rec"], recorded["pl"]
    assert len(rec) == 2
    for i, t in enumerate((1, 2)):
        e, user = rec.entry(i)
        assert (e.ticket, e.sequence, e.n_frames, e.batch_frames) == (t, t, 2, N)
        assert (e.w, e.h, e.w_bytes, e.stride, e.lag, e.input_format, e.sample_bits, e.stages) == (W, H, 3 * W, 3 * W, 3, 0, 8, STAGE_ALL)
        assert list(e.frames[:2]) == CHOSEN and (e.has_keys, e.has_origins, e.win_w) == (0, 0, 0)
        assert bytes(e.params) == bytes(recorded["params"][t]) and user == b"batch %d" % t
        frames = rec.frames(i)
        assert frames.shape == (2, H, W, 3) and np.array_equal(frames, host[t][CHOSEN])
        for k in range(2):
            assert e.sizes[k] == len(rec.frame(i, k)) <= pack_bound(3 * W, H)
            assert rec.frame(i, k).tobytes() == R.pack(host[t][CHOSEN[k]].reshape(H, 3 * W), 3).tobytes()
    assert pl.get_info().host_blocking_calls == 0


def test_armours_are_those_of_a_pipeline_without_a_recorder(recorded):
    for (a, o), (b, p) in zip(recorded["got"], recorded["want"]):
        assert a.tobytes() == b.tobytes() and o.tolist() == p.tolist()
    assert sum(len(a) for a, _ in recorded["got"]) > 0


def test_freeze_keeps_the_ring_and_resume_records_again(batches, recorded):
    _, dev = batches
    rec, pl = recorded["rec"], recorded["pl"]
    before = [bytes(rec.entry(i)[0]) for i in range(2)]
    rec.freeze()
    t = pl.submit(dev[0].data_ptr(), N, H, W, default_params(), STAGE_ALL)
    pl.collect(t)
    assert len(rec) == 2 and [bytes(rec.entry(i)[0]) for i in range(2)] == before
    rec.resume()
    t = pl.submit(dev[0].data_ptr(), N, H, W, default_params(), STAGE_ALL)
    pl.collect(t)
    assert len(rec) == 2 and rec.entry(1)[0].ticket == t and rec.entry(0)[0].ticket == 2
    assert pl.get_info().host_blocking_calls == 0


def test_replay_of_the_saved_session_returns_the_recorded_frames_armours(batches, recorded, oracle):
    host, _ = batches
    for t in (1, 2):                                             # the oracle first: every recorded frame holds an armour
        for f in CHOSEN:
            p = oracle.default_params()
            p.lower_bound = 80 - t
            assert len(oracle.detect_frame(host[t][f], p)["armours"]) >= 1
    s = Session(recorded["path"])
    assert len(s) == 2
    fresh = Pipeline(device=0, depth=2, max_frames=2, max_width=W, max_height=H)
    replayed = s.replay(fresh)
    fresh.close()
    for i, t in enumerate((1, 2)):
        e, user = s.entry(i)
        assert e.ticket == t and user == b"batch %d" % t and np.array_equal(s.frames(i), host[t][CHOSEN])
        arm, offs = recorded["got"][t]
        got, goffs = replayed[i]
        for k, f in enumerate(CHOSEN):
            want = arm[offs[f]:offs[f + 1]]
            assert len(want) >= 1 and got[goffs[k]:goffs[k + 1]].tobytes() == want.tobytes()
    s.close()


def test_bayer_pipeline_records_the_mosaic_with_lag_2(batches):
    import torch
    import bayer_ref as BR
    host, _ = batches
    mosaics = [np.stack([BR.mosaic(f, BAYER_RG) for f in b]) for b in host]
    dev = [torch.from_numpy(m).cuda() for m in mosaics]
    params = [default_params() for _ in range(3)]
    plain = make_pipeline(input_format=BAYER_RG)
    want = run_three(plain, dev, params)
    plain.close()
    rec = Recorder(device=0, slots=2, max_frames=2, max_w_bytes=W, max_h=H)
    pl = make_pipeline(input_format=BAYER_RG)
    pl.set_recorder(rec, CHOSEN)
    got = run_three(pl, dev, params)
    assert len(rec) == 2
    for i, t in enumerate((1, 2)):
        e, _ = rec.entry(i)
        assert (e.ticket, e.lag, e.input_format, e.sample_bits, e.w_bytes, e.w) == (t, 2, BAYER_RG, 8, W, W)
        assert np.array_equal(rec.frames(i), mosaics[t][CHOSEN])
    for (a, o), (b, p) in zip(got, want):
        assert a.tobytes() == b.tobytes() and o.tolist() == p.tolist()
    assert pl.get_info().host_blocking_calls == 0
    pl.close()
    rec.close()


def test_camps_and_windows_are_recorded_as_the_batch_used_them(batches):
    import torch
    host, dev = batches
    camps = np.array([1, 0, 2, 0], np.int32)
    origins = np.array([[5, 3], [100, 60], [-4, 200], [37, 11]], np.int32)
    d_camps, d_orig = torch.from_numpy(camps).cuda(), torch.from_numpy(origins).cuda()
    params = [default_params() for _ in range(3)]
    for kw in ({"camps": (d_camps.data_ptr(), None)}, {"windows": (d_orig.data_ptr(), 64, 48)}):
        plain = make_pipeline()
        want = run_three(plain, dev, params, **kw)
        plain.close()
        rec = Recorder(device=0, slots=2, max_frames=2, max_w_bytes=3 * W, max_h=H)
        pl = make_pipeline()
        pl.set_recorder(rec, CHOSEN)
        got = run_three(pl, dev, params, **kw)
        cx = pl.context_of(2)
        e, _ = rec.entry(1)
        assert e.ticket == 2 and np.array_equal(rec.frames(1), host[2][CHOSEN])      # the frames as delivered, whole
        if "camps" in kw:
            keys = cx.frame_keys()
            assert e.has_keys == 1 and e.has_origins == 0
            assert np.array_equal(np.array([list(e.keys[k]) for k in range(2)]), keys[CHOSEN])
            assert [e.camps[k] for k in range(2)] == camps[CHOSEN].tolist()
        else:
            eff, ww, wh = cx.windows()
            assert e.has_origins == 1 and (e.win_w, e.win_h) == (ww, wh) == (64, 48)
            assert np.array_equal(np.array([list(e.origins[k]) for k in range(2)]), eff[CHOSEN])
        for (a, o), (b, p) in zip(got, want):
            assert a.tobytes() == b.tobytes() and o.tolist() == p.tolist()
        assert pl.get_info().host_blocking_calls == 0
        pl.close()
        rec.close()


def test_refusals_come_before_anything_is_enqueued(batches):
    _, dev = batches
    rec = Recorder(device=0, slots=2, max_frames=2, max_w_bytes=3 * W, max_h=H)
    small = Recorder(device=0, slots=2, max_frames=2, max_w_bytes=100, max_h=H)
    pl = Pipeline(device=0, depth=2, max_frames=8, max_width=W, max_height=H)
    for frames in ([0, 0], [0, 8], [-1], [0, 1, 2]):               # repeated; beyond the pipeline; negative; more than the recorder holds
        with pytest.raises(RmcvError) as e:
            pl.set_recorder(rec, frames)
        assert e.value.code == abi.ERR_BAD_ARG
    for r, frames in ((rec, [0, 5]), (small, [0, 3])):              # an index beyond the batch; a geometry beyond the recorder
        pl.set_recorder(r, frames)
        with pytest.raises(RmcvError) as e:
            pl.submit(dev[0].data_ptr(), N, H, W, default_params(), STAGE_ALL)
        assert e.value.code == abi.ERR_BAD_ARG
        assert pl.get_info().submitted == 0 and len(r) == 0
    pl.set_recorder(None, [])                                      # off: a submit is what it was
    pl.collect(pl.submit(dev[0].data_ptr(), N, H, W, default_params(), STAGE_ALL))
    assert len(rec) == 0 and len(small) == 0
    pl.close()
    rec.close()
    small.close()


def test_stand_alone_record_and_device_frame(bufs):
    planes = np.stack([R.plane(k, 300, 17, seed=1) for k in ("poisson", "ramp", "bright")])
    bufs["in"].put(planes)
    rec = Recorder(device=0, slots=3, max_frames=2, max_w_bytes=300, max_h=17)
    rec.record(bufs["in"].p, 300, 17, lag=2, frames=[2, 0])
    assert len(rec) == 1
    e, user = rec.entry(0)
    assert (e.ticket, e.n_frames, e.batch_frames, e.lag, e.input_format, user) == (0, 2, 3, 2, -1, b"")
    assert np.array_equal(rec.frames(0), planes[[2, 0]])
    d, size = rec.device_frame(0, 1)
    assert d and size == len(R.pack(planes[0], 2))
    with pytest.raises(RmcvError):
        rec.record(bufs["in"].p, 301, 17, lag=2, n=1)              # beyond the recorder's rows
    rec.close()
