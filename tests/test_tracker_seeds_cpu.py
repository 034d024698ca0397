"""The seeded cases of tests/track_seeds.py on the CPU: every case's list stepped by rmcv_tracker_step_host (the source k_track is
compiled from) and by a seeded RefStream (the oracle's tracker with only hypot pinned) -- tracks, side records, status and origin byte
for byte -- and every case's branch census asserted on the reference's own run: each case reaches the branch it is named for.  Inputs are
the oracle's detection of each frame (of the crop at the effective origin for the windowed cases), identities from its classifier with
the synthetic SVM, poses from its locate_armours.  Three chained steps per stream: the frame, black, the frame again."""
import numpy as np
import pytest

import track_seeds as K
import window_ref as W
from rmcv_amd import abi, synth


@pytest.fixture(scope="module")
def observed(oracle):
    """case name -> Obs of its frame by the oracle (computed once, read-only)"""
    svm = synth.svm_weights()
    out = {}
    for c in K.CASES:
        eff = K.effective_origin(c)
        f = K.frame(c.frame)
        img = f if c.request is None else W.crop(f, eff, K.WW, K.WH)
        arm = oracle.detect_frame(img, oracle.default_params())["armours"]
        ids = oracle.classify_armours(img, arm, svm)[0].astype(np.int32)
        pos = oracle.locate_armours(abi.armours_to_frame(arm, *eff))[2].copy()
        for a in (arm, ids, pos):
            a.setflags(write=False)
        out[c.name] = K.Obs(arm, ids, pos, eff)
    return out


def nothing(obs):
    return K.Obs(np.zeros(0, abi.ARMOUR), np.zeros(0, np.int32), np.zeros((0, 3)), obs.eff)


def test_the_frames_hold_what_the_cases_rely_on(observed):
    n = {k: len(o.armours) for k, o in observed.items()}
    assert all(9 <= n[k] <= 40 for k in ("many_match", "many_fresh", "mixed", "cap_exact", "cap_plus_one", "bare")), n
    assert all(65 <= n[k] <= 128 for k in ("flood_early_0", "flood_early_2", "flood_walk")), n
    assert n["identities"] == 6 and n["cap4_applied"] == 3 and n["cap1_walk"] == 2 and n["cap1_applied"] == 1 and n["win_silent"] == 0
    # an armour pair of tile4 competes for one seed's box
    assert K.overlapping_pair(abi.armours_to_frame(observed["mixed"].armours, 0, 0)) is not None
    # the windowed cases that see armours add a non-zero (fx, fy); no requested x is a multiple of 16, two origins lie partly outside
    win = [c for c in K.CASES if c.request is not None]
    assert all(c.request[0] % 16 for c in win) and sum(1 for c in win if not (0 <= c.request[0] <= K.FW - K.WW and 0 <= c.request[1] <= K.FH - K.WH)) >= 2
    assert all(min(observed[c.name].eff) > 0 for c in win if n[c.name])
    assert {c.group for c in K.CASES} == set(K.GROUPS)


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_seeded_case_step_host_equals_the_reference_and_reaches_its_branch(case, observed):
    obs = observed[case.name]
    s = K.Stream(case)
    s.put(*s.seed(obs, K.STAMPS[0]))
    seeded = s.state()
    c = s.step(obs, K.STAMPS[0])                       # (asserts step_host == RefStream byte for byte)
    case.check(c)
    assert (case.name in K.REFUSED) == c["refused"]
    if c["refused"]:
        assert s.state()[:2] == seeded[:2] and s.state()[3] == K.ORIGIN0 and s.ref.status == 1
    if case.group == "bare":
        assert s.ref.origin == K.ORIGIN0                # win_w == 0: the origin stays
    elif not c["refused"]:
        assert s.ref.origin != K.ORIGIN0                # rewritten, on a step without observations too
    if case.build is K.b_silent:                       # from the LOWER index of the two newest seeds
        assert s.ref.origin == abi.window_origin(abi.get_roi(s.ref.side[1], (s.cfg.roi_scale_w, s.cfg.roi_scale_h), (K.FW, K.FH)), K.WW, K.WH)
    after1 = s.state()
    c2 = s.step(nothing(obs), K.STAMPS[1])             # black: no observation -- nothing ages, nothing is refused
    assert not c2["applied"] and not c2["refused"] and s.state()[:3] == after1[:3]
    after2 = s.state()                                 # (the origin was recomputed: a step without observations still does that)
    c3 = s.step(obs, K.STAMPS[2])
    if c3["refused"]:
        assert s.state() == after2
    elif c3["n_obs"]:
        assert c3["applied"] and s.state()[0] != after1[0]
        assert c3["matches"] + c3["fresh"] == c3["n_obs"] and (s.ref.tracks["timestamp"] == K.STAMPS[2]).sum() == c3["n_obs"]
    assert s.ref.status == (1 if c["refused"] or c3["refused"] else 0)
