"""The leaf functions of rmcv_amd/csrc/pinned_math.h and enhance_math.h without a GPU, over the case list of tests/leaf_cases.py:

a. the gcc build (tests/leaf/leaf_host_main.c, gcc -O2 -ffp-contract=off -fno-fast-math: how the CPU oracle and the tests' references are
   built) against hipcc's clang host pass (tests/leaf/leaf_main.hip --host-only: how the library's own host entry points are built), bit
   for bit on every record -- tests/test_gpu_leaf.py adds the device as the third build;
b. the comparison rule both files use;
c. the accuracy against TRUE values (mpmath, 200 bits), in ulps of the true value.  The bounds are not taken from the code under test:
   sin, cos, tan, acos below 1 ulp and hypot correctly rounded are pinned_math.h's own claims; atan, atan2, log, exp at most 2 ulp is what
   a correctly rounded quotient, a kernel below 1 ulp and one final addition can add up to; pow's relative error is at most
   (2.5 |g ln x| + 2) 2^-53 per input (a 2 ulp logarithm and a half-ulp product carried into the exponent, then exp's own 2 ulp); the float
   variants equal mpmath's correctly rounded float except at most once in 2^20 results, and on the 16 641 lattice pairs of contour points
   always;
d. the same host loops under -fsanitize=undefined,float-cast-overflow, as a stand-alone program run as a child process (nothing is loaded
   into python): clean over the whole list, the arguments beyond the range of pm_rem_pio2's conversion included.

Measured on this list (max error in ulp of the true value): sin 0.785, cos 0.804, tan 0.754, acos 0.833, atan 0.743, atan2 1.255, log 0.783,
exp 1.088; hypot, the lattice and the float variants without a single miss; pow, over all 2 011 575 pairs of the list with |g ln x| <= 700,
987 x 2^-53 at (i, gamma) = (140, 1000), |g ln x| = 600, and never more than 0.842 of a pair's own bound (at (93, 15.98)).  Before pm_log
summed from the exact m - 1 it held 1.87 ulp, and pm_pow was 7 % over its bound at (i, gamma) = (177, 400)."""
import math
import os
import subprocess

import mpmath
import numpy as np
import pytest

import leaf_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST_SRC = os.path.join(HERE, "leaf", "leaf_host_main.c")
GCC_FLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math"]
SAN_FLAGS = ["-x", "c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all",
             "-fno-omit-frame-pointer"]
mpmath.mp.prec = 200


def build_gcc_program(directory):
    exe = os.path.join(str(directory), "leaf_host_main")
    subprocess.run(["gcc"] + GCC_FLAGS + [HOST_SRC, "-o", exe, "-lm"], check=True)
    return exe


def build_leaf_main():
    """the Makefile's own target: the library's $(CXXFLAGS), into tests/_build/"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "rmcv_amd", "csrc"), "-j", "1", "leaf"], check=True)
    return os.path.join(HERE, "_build", "leaf_main")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """{'gcc': results, 'clang': results, 'dir', 'cases'}: each program run once over the whole list"""
    d = tmp_path_factory.mktemp("leaf")
    recs = K.records()
    cases = str(d / "cases.bin")
    K.write_case_file(cases, recs)
    out = {"dir": d, "cases": cases}
    for name, cmd in (("gcc", [build_gcc_program(d)]), ("clang", [build_leaf_main(), "--host-only"])):
        dst = str(d / (name + ".bin"))
        done = subprocess.run(cmd + [cases, dst], capture_output=True, text=True)
        assert done.returncode == 0, (name, done.stderr)
        out[name] = [host for _, host in K.read_result_file(dst, recs)]
    return out


def report(rec, a, b, what):
    bad = K.different(a, b, rec.out_kind)
    if len(bad) == 0:
        return None
    i = int(bad[0])
    return "%s: %d of %d differ (%s); first at %d: args %s -> %016x / %016x" % (rec.name, len(bad), len(rec), what, i, [hex(int(s[i])) for s in rec.args],
                                                                                int(a[i]), int(b[i]))


# ---------------------------------------------------------------- a. gcc against clang
def test_the_list_is_what_it_says():
    recs = K.records()
    total = sum(len(r) for r in recs)
    print("%d records, %d elements" % (len(recs), total))
    assert {r.func for r in recs} == set(K.FUNCS) and len({r.name for r in recs}) == len(recs)
    assert [r.name for r in recs if r.edge] == ["sin/edge", "cos/edge", "tan/edge"]
    x = recs[0].values(0)
    assert recs[0].name == "sin/domain" and np.abs(x).max() <= 1e4
    fm = next(r for r in recs if r.func == "fmod180").values(0)
    assert (((fm >= 0) & (fm < 720)) | np.isnan(fm)).all()                      # nothing else may reach pm_fmod180's loop
    lat = next(r for r in recs if r.name == "atan2f/lattice")
    assert len(lat) == 16641


@pytest.mark.parametrize("func", K.functions())
def test_gcc_and_clang_host_builds_give_the_same_bits(run, func):
    failures = [report(r, run["gcc"][k], run["clang"][k], "gcc / clang host") for k, r in enumerate(K.records()) if r.func == func]
    assert not any(failures), [f for f in failures if f]


# ---------------------------------------------------------------- b. the rule
def test_comparison_rule():
    nan_a, nan_b = 0x7FF8000000000000, 0xFFF800000000BEEF                      # two NaNs: equal whatever their sign and payload
    a = np.array([nan_a, 0x0000000000000000, 0x3FF0000000000000, nan_a], np.uint64)
    b = np.array([nan_b, 0x8000000000000000, 0x3FF0000000000001, 0x7FF0000000000000], np.uint64)
    assert K.different(a, b, "f64").tolist() == [1, 2, 3]                      # +0 / -0, one ulp, NaN / infinity: all differ
    fa, fb = np.array([0x7FC00000, 0x00000000, 0x7FC00000], np.uint64), np.array([0xFFC00001, 0x80000000, 0x7F800000], np.uint64)
    assert K.different(fa, fb, "f32").tolist() == [1, 2]
    assert K.different(np.array([5, 0xFFFFFFFF], np.uint64), np.array([5, 0x7FFFFFFF], np.uint64), "int").tolist() == [1]


# ---------------------------------------------------------------- c. accuracy against mpmath
def correctly_rounded(v, prec=53, lsb_min=-1074):
    """the mpf v rounded ONCE to a binary format (round to nearest even, subnormals on the format's own grid), as a Python float"""
    if not mpmath.isfinite(v):
        return float(v)
    sign, man, exp, bc = v._mpf_
    if man == 0:
        return 0.0
    man = int(man)
    lsb = max(exp + bc - prec, lsb_min)
    shift = lsb - exp
    if shift <= 0:
        q = man << -shift
    else:
        q, r, half = man >> shift, man & ((1 << shift) - 1), 1 << (shift - 1)
        if r > half or (r == half and q & 1):
            q += 1
    try:
        out = math.ldexp(q, lsb)
    except OverflowError:
        out = math.inf
    return -out if sign else out


def ulp_error(got, true):
    """|got - true| in ulps of the true value (the ulp of a subnormal is 2^-1074)"""
    if true == 0:
        return 0.0 if got == 0 else math.inf
    _, _, exp, bc = true._mpf_
    return float(mpmath.ldexp(abs(mpmath.mpf(got) - true), -(max(exp + bc - 1, -1022) - 52)))


def worst_ulp(func, got, args, true_fn, keep):
    worst, at = 0.0, None
    for i in np.nonzero(keep)[0]:
        a = [float(v[i]) for v in args]
        e = ulp_error(float(got[i]), true_fn(*[mpmath.mpf(v) for v in a]))
        if e > worst:
            worst, at = e, a
    print("%s: max error %.3f ulp of the true value at %s (%d arguments)" % (func, worst, [v.hex() for v in at] if at else None, int(np.count_nonzero(keep))))
    return worst


def domain_records(run, func):
    return [(r, K.from_slots(run["gcc"][k], r.out_kind)) for k, r in enumerate(K.records()) if r.func == func and not r.edge]


TRUE = {"sin": mpmath.sin, "cos": mpmath.cos, "tan": mpmath.tan, "acos": mpmath.acos, "atan": mpmath.atan, "atan2": mpmath.atan2, "log": mpmath.log,
        "exp": mpmath.exp}


@pytest.mark.parametrize("func,bound", [("sin", 1.0), ("cos", 1.0), ("tan", 1.0), ("acos", 1.0)])
def test_below_one_ulp_of_the_true_value(run, func, bound):
    (rec, got), = domain_records(run, func)
    x = rec.values(0)
    keep = np.abs(x) <= (1.0 if func == "acos" else 1e4)
    if func == "acos":
        assert (~keep).sum() >= 8 and np.isnan(got[~keep]).all()                # |x| > 1 and NaN: NaN
    else:
        assert keep.all()
    assert worst_ulp(func, got, [x], TRUE[func], keep) < bound


@pytest.mark.parametrize("func", ["atan", "atan2", "log", "exp"])
def test_at_most_two_ulp_of_the_true_value(run, func):
    worst = 0.0
    for rec, got in domain_records(run, func):
        args = [rec.values(k) for k in range(len(rec.args))]
        if func == "atan":
            keep = ~np.isnan(args[0])
        elif func == "atan2":
            keep = np.isfinite(args[0]) & np.isfinite(args[1]) & (args[0] != 0) & (args[1] != 0)
        elif func == "log":
            keep = (args[0] >= K.DBL_MIN) & np.isfinite(args[0])
            if rec.name == "log/outside":
                keep &= False
        else:
            keep = (args[0] >= -708.0) & (args[0] <= 709.0)
        worst = max(worst, worst_ulp(rec.name, got, args, TRUE[func], keep))
    assert worst <= 2.0


def test_hypot_equals_the_correctly_rounded_value(run):
    (rec, got), = domain_records(run, "hypot")
    x, y = rec.values(0), rec.values(1)
    keep = np.isfinite(x) & np.isfinite(y)
    assert np.count_nonzero(keep) > 50000
    bad = []
    for i in np.nonzero(keep)[0]:
        a, b = mpmath.mpf(float(x[i])), mpmath.mpf(float(y[i]))
        want = correctly_rounded(mpmath.sqrt(mpmath.fadd(mpmath.fmul(a, a, exact=True), mpmath.fmul(b, b, exact=True), exact=True)))
        if float(got[i]) != want:
            bad.append((float(x[i]).hex(), float(y[i]).hex(), float(got[i]).hex(), want.hex()))
    assert not bad, (len(bad), bad[:5])


def pow_chunk(x, g, got):
    """pm_pow's results for the pairs (x, g) against mpmath, every pair against its own bound
    -> (pairs measured, [max relative error in 2^-53, (i, gamma, |g ln x|)], [largest fraction of the bound, (i, gamma)], pairs over the bound)"""
    mpmath.mp.prec = 200                                                        # a worker process starts from the default
    eps, logs = mpmath.ldexp(1, -53), {}
    n, worst, closest, over = 0, [0.0, None], [0.0, None], []
    for x, g, got in zip(x.tolist(), g.tolist(), got.tolist()):
        i = round(x * 255.0)
        if x == 0.0 or g == 0.0:
            assert got == (1.0 if g == 0.0 else 0.0), (i, g, got)
            continue
        if x not in logs:
            logs[x] = mpmath.log(mpmath.mpf(x))
        gl = mpmath.mpf(g) * logs[x]
        if abs(gl) > 700:                                                       # beyond the normal range: 0 by contract, not by accuracy
            continue
        true = mpmath.exp(gl)
        rel = abs(mpmath.mpf(got) - true) / true
        bound = (2.5 * abs(gl) + 2) * eps
        n += 1
        if rel / eps > worst[0]:
            worst = [float(rel / eps), (i, g, float(abs(gl)))]
        if rel / bound > closest[0]:
            closest = [float(rel / bound), (i, g)]
        if rel > bound:
            over.append((i, g, got, float(rel), float(bound)))
    return n, worst, closest, over


def test_pow_relative_error_bound(run):
    """every i against every gamma of the list, two million pairs: mpmath takes about two CPU minutes for them, so the pairs are dealt out
    to a few fresh worker processes (spawned, not forked: they share nothing with this one but the arrays they are sent)"""
    import concurrent.futures
    import multiprocessing
    workers = max(1, min(8, len(os.sched_getaffinity(0))))
    jobs = []
    for rec, got in domain_records(run, "pow"):
        assert len(rec) == 256 * len(K.gammas()[rec.name == "pow/uniform"])     # nothing of the list is left out
        x, g = rec.values(0), rec.values(1)
        jobs += [(x[a:a + 65536], g[a:a + 65536], got[a:a + 65536]) for a in range(0, len(rec), 65536)]
    with concurrent.futures.ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("spawn")) as pool:
        parts = list(pool.map(pow_chunk, *zip(*jobs)))
    n = sum(p[0] for p in parts)
    worst, closest = max((p[1] for p in parts), key=lambda w: w[0]), max((p[2] for p in parts), key=lambda w: w[0])
    over = [o for p in parts for o in p[3]]
    print("pow: max relative error %.1f x 2^-53 at (i, gamma, |g ln x|) = %s; at most %.3f of the bound, at (i, gamma) = %s; %d of %d pairs over it"
          % (worst[0], worst[1], closest[0], closest[1], len(over), n))
    assert n > 2000000
    assert not over, (len(over), over[:5])


def float_misses(rec, got, true_fn):
    args = [rec.values(k) for k in range(len(rec.args))]
    keep = np.ones(len(rec), bool)
    for a in args:
        keep &= np.isfinite(a)
    bad = []
    for i in np.nonzero(keep)[0]:
        a = [float(v[i]) for v in args]
        want = correctly_rounded(true_fn(*[mpmath.mpf(v) for v in a]), 24, -149)
        if float(got[i]) != want:
            bad.append((a, float(got[i]), want))
    print("%s: %d of %d results are not the correctly rounded float" % (rec.name, len(bad), int(np.count_nonzero(keep))))
    return bad, int(np.count_nonzero(keep))


@pytest.mark.parametrize("func,true_fn", [("atan2f", mpmath.atan2), ("sinf", mpmath.sin), ("cosf", mpmath.cos)])
def test_float_variants_are_the_correctly_rounded_float(run, func, true_fn):
    for rec, got in domain_records(run, func):
        bad, n = float_misses(rec, got, true_fn)
        allowed = 0 if rec.name == "atan2f/lattice" else n >> 20                # at most 1 in 2^20; the lattice gets no allowance
        assert len(bad) <= allowed, (rec.name, len(bad), bad[:5])


def test_fmod180_is_fmod(run):
    (rec, got), = domain_records(run, "fmod180")
    x = rec.values(0)
    want = np.fmod(x, 180.0)
    assert not len(K.different(K.to_slots(got, "f64"), K.to_slots(want, "f64"), "f64"))


def test_beyond_the_conversion_the_answer_is_nan(run):
    """pm_rem_pio2's quadrant number is an int: where |x * invpio2| >= 2^31 - 1, and for infinities and NaN, sin, cos and tan are NaN on every
    build; below that they are finite, and sine and cosine stay within [-1, 1] (no 7e121)"""
    for k, r in enumerate(K.records()):
        if not r.edge:
            continue
        x, got = r.values(0), K.from_slots(run["gcc"][k], "f64")
        out = ~(np.abs(x * K.INVPIO2) < 2147483647.0)
        assert out.sum() > 1000 and (~out).sum() > 1000
        assert np.isnan(got[out]).all(), r.name
        assert np.isfinite(got[~out]).all(), r.name
        if r.func != "tan":
            assert np.abs(got[~out]).max() <= 1.0, r.name
        # the edge itself, in numbers that do not come from the code: 2^31 pi / 2 = 3.3732e9 lies between these two
        for v, refused in ((3.37e9, False), (-3.37e9, False), (3.38e9, True), (-3.38e9, True), (1e10, True), (K.packet_radians(1e12), True),
                           (K.packet_radians(-1e12), True), (K.packet_radians(K.FLT_MAX), True), (math.inf, True), (-math.inf, True)):
            at = np.nonzero(x == v)[0]
            assert len(at) and (np.isnan(got[at]) if refused else np.isfinite(got[at])).all(), (r.name, v)
        assert np.isnan(got[np.isnan(x)]).all() and np.isnan(x).any()


# ---------------------------------------------------------------- d. sanitized
def test_host_loops_under_the_sanitizer(run):
    exe = os.path.join(str(run["dir"]), "leaf_san_main")
    subprocess.run(["g++"] + SAN_FLAGS + [HOST_SRC, "-o", exe], check=True)
    dst = os.path.join(str(run["dir"]), "san.bin")
    done = subprocess.run([exe, run["cases"], dst], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert done.returncode == 0, done.stderr[-2000:]
    recs = K.records()
    for (_, host), want, r in zip(K.read_result_file(dst, recs), run["gcc"], recs):
        assert report(r, host, want, "sanitized g++ -O1 / gcc -O2") is None
