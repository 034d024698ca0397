"""pixel_set_for and pixel_set_waits (rmcv_amd/csrc/pixel_sets_plan.h): which of a hot context's two pixel-output sets a batch takes and
what its streams wait for.  Compiled with the host C++ compiler and checked against a Python restatement for hot = 3 .. 7, fast and not
fast, contexts with and without a second set, changed and unchanged geometry; then the property the sets exist for: consecutive visits
of a context alternate, so the last batch in the same set lies 2 hot batches back."""
import itertools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stdio.h>
#include "rmcv_amd/csrc/pixel_sets_plan.h"
using namespace rmcv;
int main()
{
    for (int fast = 0; fast < 2; fast++)
    for (int sets = 1; sets <= 2; sets++)
    for (int hot = 0; hot <= 7; hot = hot ? hot + 1 : 3)
    for (unsigned long long seq = 0; seq < 40; seq++)
        printf("set %d %d %d %llu : %d\n", fast, sets, hot, seq, pixel_set_for(fast != 0, seq, hot, sets));
    for (int fast = 0; fast < 2; fast++)
    for (int sets = 1; sets <= 2; sets++)
    for (int changed = 0; changed < 2; changed++) {
        const SetWaits w = pixel_set_waits(fast != 0, sets, changed != 0);
        printf("wait %d %d %d : %d %d %d %d\n", fast, sets, changed, (int)w.pixel_ctx_last, (int)w.pixel_set_last, (int)w.pixel_ctx_bin, (int)w.sparse_ctx_last);
    }
    return 0;
}
'''


def set_for(fast, sets, hot, seq):
    """the rotation's laps alternate between the two sets; everything else takes set 0"""
    return (seq // hot) % 2 if fast and hot > 0 and sets == 2 else 0


def waits(fast, sets, changed):
    """(pixel stream: the context's last batch | the set's last batch | the context's last pixel kernel, sparse stream: the context's last batch)
    the old wait wherever there is one set, the batch is not fast, or the binding enqueues work; the sparse stream always waits"""
    old = (not fast) or sets < 2 or changed
    return (int(old), int(not old), int(not old), 1)


def test_sets_and_waits_match_the_restatement(tmp_path):
    src = tmp_path / "pixel_sets.cpp"
    src.write_text(SRC)
    exe = tmp_path / "pixel_sets"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got_sets, got_waits = {}, {}
    for line in lines:
        key, got = line.split(":")
        kind, *args = key.split()
        (got_sets if kind == "set" else got_waits)[tuple(int(v) for v in args)] = tuple(int(v) for v in got.split())
    assert set(got_sets) == set(itertools.product((0, 1), (1, 2), (0, 3, 4, 5, 6, 7), range(40)))
    for args, got in got_sets.items():
        assert got == (set_for(*args),), (args, got)
    assert set(got_waits) == set(itertools.product((0, 1), (1, 2), (0, 1)))
    for args, got in got_waits.items():
        assert got == waits(*args), (args, got)
    # a fast batch waits on the pixel stream for exactly one of the two, never for both and never for neither
    assert all(g[0] + g[1] == 1 and g[1] == g[2] for g in got_waits.values())
    # the point of the sets: context j = seq % hot meets its two sets in turn, so the same (context, set) comes back after 2 hot batches
    for hot in range(3, 8):
        last = {}
        for seq in range(40):
            j, s = seq % hot, got_sets[(1, 2, hot, seq)][0]
            if (j, 1 - s) in last:
                assert last[(j, 1 - s)] == seq - hot
            if (j, s) in last:
                assert last[(j, s)] == seq - 2 * hot
            last[(j, s)] = seq
