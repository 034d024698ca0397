"""device_harvest.h (rmcv_amd/csrc), the dataset harvest's rule, compiled by the host compiler, against its restatement in numpy
(tests/harvest_ref.py): seeded tables of 1, 63, 64, 65, 256, 257 and 1000 frames; counts that are 0, 1, max_armours and beyond it; skip
labels; each RMCV_FRAME_OVF_* status bit; both flag values; a capacity that falls before, inside and after a frame's rows, and a dataset
that is already full.  Slots, count and dropped are equal everywhere.  The library's rmcv_harvest_plan_host gives the same answers."""
import os
import subprocess

import numpy as np

import harvest_cases as K
import harvest_ref as R
import rmcv_amd

HERE = os.path.dirname(os.path.abspath(__file__))


def test_header_on_the_host_equals_the_restatement(tmp_path):
    exe = str(tmp_path / "harvest_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(HERE, "harvest_san_main.cpp"), "-o", exe], check=True)
    cs = K.calls()
    assert sorted(set(len(c[0]) for c in cs)) == list(K.FRAMES) and set(c[5] for c in cs) == {0, R.MISSES}
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(src, "wb").write(K.encode(cs))
    subprocess.run([exe, src, dst], check=True)
    K.check(K.decode(open(dst, "rb").read(), cs), cs)


def test_library_entry_point_equals_the_restatement():
    for n, st, lb, ident, ma, flags, count, cap, dropped in K.calls():
        items, now, drop = rmcv_amd.harvest_plan(n, st, lb, ident, max_armours=ma, flags=flags, count=count, capacity=cap, dropped=dropped)
        want = R.plan(n, st, lb, ident, ma, flags, count, cap, dropped)
        assert np.array_equal(items, want[0]) and (now, drop) == want[1:]


def test_library_entry_point_refusals():
    n, st, lb, ident = R.tables(8, 4, 5)
    for kw in ({"flags": 2}, {"capacity": 0}, {"count": 9, "capacity": 8}, {"flags": R.MISSES, "identity": None}):
        args = {"identity": ident, "max_armours": 4, "flags": 0, "count": 0, "capacity": 8}
        args.update(kw)
        try:
            rmcv_amd.harvest_plan(n, st, lb, **args)
        except rmcv_amd.RmcvError as e:
            assert e.code == rmcv_amd.abi.ERR_BAD_ARG
        else:
            raise AssertionError("not refused: %r" % kw)


REFUSAL_SRC = r'''
#include <stdio.h>
#include <initializer_list>
#include "rmcv_amd/csrc/device_harvest.h"
int main()
{
    for (int bound = 0; bound < 2; bound++)
    for (int stages : {0, 7, 15, 31})
    for (int flags = 0; flags < 4; flags++)
    for (int other = 0; other < 2; other++) {
        const char* why = rmcv::harvest_refusal(bound != 0, stages, flags, 0, other);
        printf("%d %d %d %d|%s\n", bound, stages, flags, other, why ? why : "");
    }
    return 0;
}
'''


def test_append_refusals_and_their_order(tmp_path):
    """what an append refuses, decided by the header before anything is enqueued: unknown flags, a dataset of another device (a machine
    with one GPU cannot reach that one through the entry points), no frames bound, a run without RMCV_STAGE_ARMOURS, RMCV_HARVEST_MISSES
    without RMCV_STAGE_IDENTITY"""
    (tmp_path / "refusals.cpp").write_text(REFUSAL_SRC)
    exe = str(tmp_path / "refusals")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.dirname(HERE), str(tmp_path / "refusals.cpp"), "-o", exe], check=True)
    seen = set()
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        key, why = line.split("|")
        bound, stages, flags, other = (int(v) for v in key.split())
        want = ("harvest: unknown flags" if flags & ~R.MISSES else
                "harvest: the dataset belongs to another device" if other else
                "harvest: no frames bound" if not bound else
                "harvest: the batch's last run lacked RMCV_STAGE_ARMOURS" if not stages & 8 else
                "harvest: RMCV_HARVEST_MISSES needs a run with RMCV_STAGE_IDENTITY" if flags & R.MISSES and not stages & 16 else "")
        assert why == want, line
        seen.add(why)
    assert len(seen) == 6
