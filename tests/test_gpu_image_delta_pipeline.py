"""Delta stores of the byte image (image_plan.h) where the steps run them: a pipeline whose calm batches take turns at four contexts, so
that every context stores its image over the one another batch left there four tickets earlier.  Twelve distinct small batches; every
ticket's image (read from its context before a later batch can take that context) and armour lists equal the oracle's.

A ticket's image can only be read while its context is still its own: a calm batch takes the next of the four hot contexts whichever slot
it is in, and rmcv_pipeline_context_of refuses a ticket whose context a later batch has taken.  So the first pass submits and collects one
batch at a time and compares EVERY ticket's image; the second pass keeps eight batches in flight, where only the lists of every ticket
and the image of the last one (nothing ran behind it) can be compared."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from rmcv_amd import STAGE_ALL, Pipeline, default_params
from rmcv_amd import abi

from test_gpu_image_delta import scene

pytestmark = pytest.mark.gpu


def test_hot_contexts_take_turns_and_every_image_is_its_batch_s(oracle):
    import torch
    dev = torch.device("cuda", 0)
    w, h, n, hot = 192, 70, 48, 4
    pl = Pipeline(device=0, depth=8, max_frames=n, max_width=w, max_height=h, hot_contexts=hot)
    assert pl.info.depth == 8 and pl.info.hot_contexts == hot
    p = default_params()
    host = [np.array(scene(w, h, n, v)) for v in range(12)]
    with ThreadPoolExecutor(16) as ex:
        refs = [list(ex.map(lambda f: oracle.detect_frame(f, p), fr)) for fr in host]
    devf = [torch.from_numpy(fr).to(dev) for fr in host]
    d0 = abi.lib().rmcv_pixel_image_delta_launches()

    def check(t, k, image=True):
        arm, offs = pl.collect(t)
        c = pl.context_of(t) if image else None                  # (refused once a later batch has taken the context)
        for f, r in enumerate(refs[k]):
            if image:
                got = c.binary(f)
                assert np.array_equal(got, r["binary"]), "ticket %d frame %d: %d bytes differ (%d stale)" % (
                    t, f, int(np.count_nonzero(got != r["binary"])), int(np.count_nonzero((got != 0) & (r["binary"] == 0))))
            assert arm[offs[f]:offs[f + 1]].tobytes() == r["armours"].tobytes(), (t, f)

    # one at a time: a ticket's context is looked at before any later batch can take it (a calm batch takes the next of the four,
    # whichever slot it is in)
    for i in range(12):
        t = pl.submit(devf[i].data_ptr(), n, h, w, p, STAGE_ALL)
        assert t == i
        check(t, i)
    # ... and with eight in flight, in another order: every list, and the image of the last ticket (nothing ran behind it)
    order = [(5 * i + 3) % 12 for i in range(12)]
    for i, k in enumerate(order):
        t = pl.submit(devf[k].data_ptr(), n, h, w, p, STAGE_ALL)
        assert t == 12 + i
        if i >= 7:
            check(t - 7, order[i - 7], image=False)
    pl.drain()
    for i in range(5, 12):
        check(12 + i, order[i], image=i == 11)
    info = pl.get_info()
    assert info.hot_batches > 0
    assert abi.lib().rmcv_pixel_image_delta_launches() - d0 > 0
    pl.close()
