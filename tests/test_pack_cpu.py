"""The session recorder's packed format on the CPU: rmcv_pack_host equals the numpy restatement of the specification
(tests/pack_ref.py) byte for byte and round-trips through rmcv_unpack_host on every shape, lag and kind of input of the case list; the sizes
the specification derives hold exactly; a buffer that does not agree with its geometry is refused; a session file round-trips, entries and
user blobs included.  No GPU: the host entry points need no device."""
import ctypes as C
import os

import numpy as np
import pytest

import pack_ref as R
from rmcv_amd import abi, pack, pack_bound, unpack
from rmcv_amd.abi import RecordEntry, RmcvError, lib, ptr
from rmcv_amd.recorder import Session

CASES = R.cases()


def test_the_restatement_round_trips_through_itself():
    for kind, w, h, lag in CASES[::7]:
        a = R.plane(kind, w, h)
        assert np.array_equal(R.unpack(R.packed(kind, w, h, lag), w, h, lag), a), (kind, w, h, lag)


@pytest.mark.parametrize("w", R.WIDTHS)
def test_pack_host_equals_the_restatement_and_round_trips(w):
    for kind, cw, h, lag in CASES:
        if cw != w:
            continue
        a = R.plane(kind, w, h)
        strided = np.full((h, w + 13), 0xEE, np.uint8)               # stride > w_bytes
        strided[:, :w] = a
        got = pack(strided[:, :w], lag)
        want = R.packed(kind, w, h, lag)
        assert got.tobytes() == want.tobytes(), (kind, w, h, lag)
        assert len(got) <= pack_bound(w, h) == R.bound(w, h)
        out = np.full((h, w + 5), 0x77, np.uint8)
        unpack(got, w, h, lag, out=out)
        assert np.array_equal(out[:, :w], a) and (out[:, w:] == 0x77).all(), (kind, w, h, lag)   # bytes beyond w_bytes untouched


@pytest.mark.parametrize("lag", (1, 2, 3, 4))
def test_sizes_the_specification_derives(lag):
    for w in R.WIDTHS:
        for h in R.HEIGHTS:
            S = R.segments(w)
            head = R.align8(h * S) + R.align8(4 * (h + 1))
            zero = pack(R.plane("zero", w, h), lag)
            assert len(zero) == head and not zero[:h * S].any()                                   # all zero: header and table alone
            # constant 0x5A: every difference is 0 except those of a row's first `lag` bytes, which have no predecessor.  A segment
            # that does not start its row is therefore predicted with b = 0; a row's first segment holds z = zigzag(0x5A) = 0xB4,
            # 8 bits against the raw value's 7: raw, b = 7
            const = pack(R.plane("constant", w, h), lag)
            seg = const[:h * S].reshape(h, S)
            assert (seg[:, 1:] == 0x10).all() and (seg[:, 0] == 7).all()
            assert len(const) == head + 32 * 7 * h
            # uniform noise: a segment with a byte >= 128 and a difference of 8 bits is raw at b = 8.  With 88 real bytes or more in every
            # segment (these widths) a segment without one has probability 2^-88: the plane packs to exactly the bound
            noise = pack(R.plane("noise", w, h), lag)
            if w in (255, 256, 480, 600):
                assert len(noise) == pack_bound(w, h) and (noise[:h * S] == 8).all()


def test_unpack_refuses_what_does_not_agree():
    a = R.plane("poisson", 300, 3)
    p = pack(a, 2)
    assert np.array_equal(unpack(p, 300, 3, 2), a)
    for bad in (p[:-1], p[:-8], np.concatenate([p, np.zeros(8, np.uint8)]), p[:10], p[:0]):
        with pytest.raises(RmcvError) as e:
            unpack(bad, 300, 3, 2)
        assert e.value.code == abi.ERR_BAD_ARG
    for w, h in ((300, 2), (300, 4), (600, 3), (256, 3)):                   # (another width with the same S is the same buffer: virtual bytes)
        with pytest.raises(RmcvError):
            unpack(p, w, h, 2)
    S = R.segments(300)
    for at, val in ((0, 9), (1, 0x18), (3 * S, 1), (R.align8(3 * S), 8), (R.align8(3 * S) + 4, 0), (R.align8(3 * S) + 12, 7)):
        q = p.copy()
        if q[at] == val:
            continue
        q[at] = val
        with pytest.raises(RmcvError):
            unpack(q, 300, 3, 2)
    assert lib().rmcv_unpack_host(None, C.c_int64(0), 300, 3, 2, ptr(a.copy()), C.c_int64(300)) == abi.ERR_BAD_ARG
    assert lib().rmcv_pack_bound(0, 1) == abi.ERR_BAD_ARG and lib().rmcv_pack_bound(1 << 20, 1 << 20) == abi.ERR_BAD_ARG
    small = np.zeros(8, np.uint8)
    size = C.c_int64(0)
    assert lib().rmcv_pack_host(ptr(a), 300, 3, C.c_int64(300), 2, ptr(small), C.c_int64(8), C.byref(size)) == abi.ERR_CAPACITY


def _entry(planes, lag, user, ticket):
    n, h, w = planes.shape
    e = RecordEntry()
    e.ticket, e.sequence, e.timestamp = ticket, ticket, 1000 + ticket
    e.n_frames, e.batch_frames, e.w, e.h, e.w_bytes, e.stride, e.lag = n, n + 1, w, h, w, w, lag
    e.input_format, e.sample_bits, e.stages, e.user_bytes = -1, 8, 15, len(user)
    e.params = abi.default_params(lower_bound=70 + ticket)
    packed = [pack(p, lag) for p in planes]
    for k in range(n):
        e.frames[k], e.sizes[k] = k + 1, len(packed[k])
    return e, packed


def test_session_file_round_trips_entries_blobs_and_frames(tmp_path):
    path = str(tmp_path / "s.rmcv")
    want = []
    for t, (kind, lag, user) in enumerate((("poisson", 3, b"first"), ("ramp", 2, b""), ("noise", 4, b"x" * 13))):
        planes = np.stack([R.plane(kind, 300, 5, seed=s) for s in range(2)])
        e, packed = _entry(planes, lag, user, t)
        arr = (C.c_void_p * 2)(*[p.ctypes.data for p in packed])
        assert lib().rmcv_session_append(path.encode(), C.byref(e), user, arr) == 0
        want.append((planes, e, user, packed))
    s = Session(path)
    assert len(s) == 3
    for i, (planes, e, user, packed) in enumerate(want):
        got, blob = s.entry(i)
        assert bytes(got) == bytes(e) and blob == user
        assert got.params.lower_bound == 70 + i and got.ticket == i and got.timestamp == 1000 + i
        for k in range(2):
            assert s.frame(i, k).tobytes() == packed[k].tobytes()
        assert np.array_equal(s.frames(i), planes)
    s.close()
    raw = open(path, "rb").read()
    assert raw[:8] == b"RMCVSESS" and int.from_bytes(raw[8:12], "little") == 1
    for cut in (len(raw) - 1, len(raw) - 9, 20, 15, 0):                      # truncated: refused
        bad = str(tmp_path / ("cut%d" % cut))
        open(bad, "wb").write(raw[:cut])
        with pytest.raises(RmcvError) as err:
            Session(bad)
        assert err.value.code == abi.ERR_BAD_ARG
    flipped = bytearray(raw)
    flipped[16] ^= 1                                                         # the first record's length word
    open(str(tmp_path / "flip"), "wb").write(bytes(flipped))
    with pytest.raises(RmcvError):
        Session(str(tmp_path / "flip"))
    assert not os.path.exists(str(tmp_path / "none")) and lib().rmcv_session_open(str(tmp_path / "none").encode(), C.byref(C.c_void_p())) == abi.ERR_BAD_ARG
