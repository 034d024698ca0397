"""Two pixel-output sets per hot context (pixel_sets_plan.h) where the steps run them: a pipeline of depth 8 whose calm batches take turns
at the hot contexts and, in each, at its two sets of bit plane, row masks, byte image and image mask.  A batch's pixel kernel then waits
for the last batch in the same set, not for the context's last one; what could go wrong is a batch's sparse stage reading a plane that a
later pixel kernel has already rewritten, a stale word under the delta stores of plane or image, or the getters reading the other set.

Five scenes in turn, one of them dark: the period is coprime to 8 and to the hot contexts, so every (context, set) meets every scene
behind a different one.  Every ticket's armour lists equal the oracle's; the newest ticket's image and contours, read through
context_of, equal the oracle's.  In mid-stream: a change of geometry and back, a batch without the image, the rotation switched off for a
ring cycle and on again.

(48 frames of 256x96 per batch: 144 strips.  With fewer strips than half the CUs the planner hands a batch to k_binary, and neither
k_binary_ws nor its delta stores would run.)"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from rmcv_amd import STAGE_ALL, STAGE_NO_IMAGE, Pipeline, default_params
from rmcv_amd import abi

from test_gpu_image_delta import flat, scene

pytestmark = pytest.mark.gpu

W, H, N = 256, 96, 48
W2, H2 = 192, 70
_cache = {}


def batches(oracle):
    """five scenes of W x H (the fourth dark) and two of W2 x H2, with the oracle's results, computed once"""
    if not _cache:
        p = default_params()
        host = [np.array(scene(W, H, N, v)) for v in (0, 1, 2)] + [np.array(flat(W, H, N, False)), np.array(scene(W, H, N, 3))]
        other = [np.array(scene(W2, H2, N, v)) for v in (0, 1)]
        with ThreadPoolExecutor(16) as ex:
            _cache["main"] = [(fr, list(ex.map(lambda f: oracle.detect_frame(f, p), fr))) for fr in host]
            _cache["other"] = [(fr, list(ex.map(lambda f: oracle.detect_frame(f, p), fr))) for fr in other]
    return _cache["main"], _cache["other"]


@pytest.mark.parametrize("hot_cfg", [4, 0], ids=["hot4", "derived"])
def test_both_sets_of_every_hot_context_serve_their_batches(oracle, hot_cfg):
    import torch
    dev = torch.device("cuda", 0)
    main, other = batches(oracle)
    pl = Pipeline(device=0, depth=8, max_frames=N, max_width=W, max_height=H, hot_contexts=hot_cfg)
    hot = pl.info.hot_contexts
    assert pl.info.depth == 8 and hot == (4 if hot_cfg else 7)       # (derived: planes this small all fit, depth - 1 contexts take turns)
    p = default_params()
    d_main = [torch.from_numpy(fr).to(dev) for fr, _ in main]
    d_other = [torch.from_numpy(fr).to(dev) for fr, _ in other]
    L = abi.lib()
    p0, i0 = L.rmcv_pixel_plane_delta_launches(), L.rmcv_pixel_image_delta_launches()
    live = {}                                                        # ticket -> (refs, (w, h), lists wanted)
    expected_hot = 0
    rotating = True
    state = {"k": 0}

    def check(t, image=False):
        refs, (w, h), stages = live.pop(t)
        arm, offs = pl.collect(t)
        for f, r in enumerate(refs):
            assert arm[offs[f]:offs[f + 1]].tobytes() == r["armours"].tobytes(), (t, f)
        if image:
            c = pl.context_of(t)
            for f, r in enumerate(refs):
                if not (stages & STAGE_NO_IMAGE):
                    got = c.binary(f)
                    assert np.array_equal(got, r["binary"]), "ticket %d frame %d: %d bytes differ (%d stale)" % (
                        t, f, int(np.count_nonzero(got != r["binary"])), int(np.count_nonzero((got != 0) & (r["binary"] == 0))))
                pts, co = c.contours(f)
                assert np.array_equal(co, r["offs"]) and np.array_equal(pts, r["pts"]), (t, f)

    def submit(which=None, stages=STAGE_ALL):
        nonlocal expected_hot
        if which is None:
            k = state["k"] % 5
            state["k"] += 1
            (fr, refs), d, (w, h) = main[k], d_main[k], (W, H)
        else:
            (fr, refs), d, (w, h) = other[which], d_other[which], (W2, H2)
        t = pl.submit(d.data_ptr(), N, h, w, p, stages)
        live[t] = (refs, (w, h), stages)
        if rotating and t > 0:
            expected_hot += 1
        if t >= 7 and (t - 7) in live:
            check(t - 7)
        return t

    # the first batch alone: its record tells the pipeline that the stream is calm, and the rotation starts with the second
    t = submit()
    check(t, image=True)
    # two laps of both sets of every context and three more, eight in flight
    for _ in range(2 * 2 * hot + 3):
        t = submit()
    check(t, image=True)                                             # the newest ticket: nothing ran behind it
    # a change of geometry and back: the binding zeroes both sets' planes behind the context's last batch
    t = submit(which=0)
    t = submit(which=1)
    check(t, image=True)
    for _ in range(hot + 1):
        t = submit()
    check(t, image=True)
    # one batch without the image: its set's plane is out of step with its image, the next batch in that set stores the whole plane
    t = submit(stages=STAGE_ALL | STAGE_NO_IMAGE)
    check(t, image=True)
    for _ in range(2 * hot + 1):
        t = submit()
    check(t, image=True)
    # the rotation off for a ring cycle -- every batch in its slot's own context, set 0 -- and on again
    pl.set_hot_contexts(0)
    rotating = False
    for _ in range(8):
        t = submit()
    check(t, image=True)
    pl.set_hot_contexts(hot)
    rotating = True
    for _ in range(2 * 2 * hot + 3):
        t = submit()
    pl.drain()
    for tt in sorted(live):
        check(tt, image=tt == t)
    info = pl.get_info()
    assert info.host_blocking_calls == 0
    assert info.hot_batches == expected_hot
    assert L.rmcv_pixel_plane_delta_launches() - p0 > 0
    assert L.rmcv_pixel_plane_delta_launches() - p0 <= L.rmcv_pixel_image_delta_launches() - i0
    for c in pl.contexts:
        assert c.check_guards()[0] == 0
    pl.close()
