"""rmcv_amd/csrc/model_plan.h against tests/model_ref.py, its restatement in numpy: the header is compiled with the host
C++ compiler (tests/models_san_main.cpp, -Wall -Werror) and asked for the rule from a raw model index to a table entry over
{-2^31, -1, 0, 1, n-1, n, 2^31-1} for n in {1, 2, 64}; the packed bytes of tables whose entries have 2, 3, 7 and 8 classes (and 1 of 2,
64 of 8); every refusal message, and which one comes first; and run_steps (bind_plan.h) with its trailing `models`.  And the Python
binding names the seven new symbols.  CPU tests: nothing here touches a GPU."""
import os
import re
import subprocess

import pytest

import model_cases as K
import model_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
NEW_SYMBOLS = ("rmcv_frame_model", "rmcv_svm_load_models", "rmcv_batch_set_frame_models", "rmcv_batch_set_device_frame_models",
               "rmcv_batch_get_frame_models", "rmcv_pipeline_set_frame_models", "rmcv_svm_predict_model")


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    d = tmp_path_factory.mktemp("model_plan")
    exe, src, dst = str(d / "model_plan"), str(d / "in.bin"), str(d / "out.bin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "models_san_main.cpp"), "-o", exe], check=True)
    open(src, "wb").write(K.encode())
    done = subprocess.run([exe, src, dst], check=True, capture_output=True, text=True)
    return done.stdout.splitlines(), open(dst, "rb").read(), K.expected()


def lines(answers, kind):
    got, _, (want, _) = answers
    return [ln for ln in got if ln[0] == kind], [ln for ln in want if ln[0] == kind]


def test_the_rule(answers):
    got, want = lines(answers, "R")
    assert len(want) == 21 and got == want
    # ... and what the restatement says is what the issue's sentence says
    assert [R.frame_model_eff(i, 2) for i in (-2**31, -1, 0, 1, 2, 2**31 - 1)] == [0, 0, 0, 1, 0, 0]
    assert R.frame_model_eff(63, 64) == 63 and R.frame_model_eff(64, 64) == 0


def test_packed_tables_byte_for_byte(answers):
    got, want = lines(answers, "T")
    _, blob, (_, want_blob) = answers
    assert sum(" : ok " in ln for ln in want) == 3 and got[:3] == want[:3]
    assert len(blob) == (1 + 4 + 64) * R.ENTRY.itemsize and blob == want_blob
    # unused decision functions and labels are zero, the stride keeps every weight row 16-byte aligned
    import numpy as np
    t = np.frombuffer(blob, R.ENTRY)
    assert t["n_class"].tolist() == [2, 2, 3, 7, 8] + [8] * 64
    assert not t[1]["weights"][1:].any() and not t[1]["rho"][1:].any() and not t[1]["labels"][2:].any() and not t["pad"].any()
    assert R.ENTRY.itemsize % 16 == 0 and (R.NFEAT * 4) % 16 == 0


def test_every_refusal_message(answers):
    got, want = lines(answers, "T")
    assert got == want
    text = "\n".join(want[3:])
    for what in ("n_models 0 is out of range (1 .. 64)", "n_models 65 is out of range", "n_models -1 is out of range", ": a null pointer", "model 1: a null pointer",
                 "model 2: n_class 1 is out of range (2 .. 8)", "model 2: n_class 9 is out of range", "model 1: weight 7 of decision function 2 is not finite",
                 "model 3: rho 27 is not finite", "model 0: rho 0 is not finite", "model 0: weight 1199 of decision function 0 is not finite"):
        assert what in text, what
    assert all(" : ok " not in ln for ln in want[3:])
    for kind, n in (("F", len(K.setter_cases())), ("P", 8)):
        g, w = lines(answers, kind)
        assert len(w) == n and g == w
    assert "frame 1: model 4 is outside the table (0 .. 3)" in "\n".join(lines(answers, "F")[1])
    assert sum(ln.endswith(": -") for ln in lines(answers, "F")[1]) == 1 and sum(ln.endswith(": -") for ln in lines(answers, "P")[1]) == 2


def test_run_steps_with_models(answers):
    got, want = lines(answers, "S")
    assert got == want == ["S 8128 0"]


def test_the_binding_names_the_new_symbols():
    from rmcv_amd import abi
    assert all(s in abi.EXPORTS for s in NEW_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "rmcv_abi.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % s, header), s
    assert re.search(r"#define RMCV_SVM_MAX_MODELS 64\b", header) and abi.SVM_MAX_MODELS == R.MAX_MODELS == 64
    assert [f[0] for f in abi.SvmModel._fields_] == ["weights", "rho", "labels", "n_class", "reserved"]
