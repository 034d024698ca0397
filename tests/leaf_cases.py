"""The case list of the leaf tests (TEST INFRASTRUCTURE), shared by tests/test_leaf_cpu.py and tests/test_gpu_leaf.py: for every function of
rmcv_amd/csrc/pinned_math.h and enhance_math.h, and for the IEEE primitives they take for granted, the arguments at which a build could part
from another -- seeded and deterministic.  tests/leaf/leaf_funcs.h holds the same table of ids; tests/leaf/leaf_main.hip says how the files
are laid out.  Every argument and result is a 64-bit slot: a double as its bits, a float as its 32 bits, an integer as itself.

Records named '<function>/edge' hold the arguments beyond the range of pm_rem_pio2's conversion to int (undefined behaviour before the
reduction refused them); every other record is in the functions' declared domain or in a range where the code is bit moves and defined.

Size: 6.5 million elements, at most 2^18 per record except the four of pow and enh_lut_entry, which hold every i in 0..255 against every
gamma (3 798 of tests/test_enhance_cpu.py, 4 096 uniform) and so about a million each.  Generating the list takes 0.3 s, and either host
build evaluates all of it in 0.3 s -- within the couple of seconds a test run may spend on it."""
import functools
import math
import struct

import numpy as np

MAGIC = 0x4641454C
# name -> (id, kinds of the argument slots, kind of the result)
FUNCS = {
    "sin": (0, ("f64",), "f64"), "cos": (1, ("f64",), "f64"), "tan": (2, ("f64",), "f64"), "atan": (3, ("f64",), "f64"),
    "atan2": (4, ("f64", "f64"), "f64"), "acos": (5, ("f64",), "f64"), "sinf": (6, ("f32",), "f32"), "cosf": (7, ("f32",), "f32"),
    "atan2f": (8, ("f32", "f32"), "f32"), "fmod180": (9, ("f64",), "f64"), "log": (10, ("f64",), "f64"), "exp": (11, ("f64",), "f64"),
    "pow": (12, ("f64", "f64"), "f64"), "hypot": (13, ("f64", "f64"), "f64"),
    "enh_gamma": (14, ("u64", "u64", "u64", "i64", "f32", "f32"), "f32"), "enh_lut_entry": (15, ("i64", "f32"), "int"),
    "sqrt64": (16, ("f64",), "f64"), "sqrt32": (17, ("f32",), "f32"), "div64": (18, ("f64", "f64"), "f64"), "div32": (19, ("f32", "f32"), "f32"),
    "fma64": (20, ("f64", "f64", "f64"), "f64"), "add32": (21, ("f32", "f32"), "f32"), "mul32": (22, ("f32", "f32"), "f32"),
    "add64": (23, ("f64", "f64"), "f64"), "mul64": (24, ("f64", "f64"), "f64"), "narrow": (25, ("f64",), "f32"),
    "i64_to_f64": (26, ("i64",), "f64"), "u64_to_f64": (27, ("u64",), "f64"), "rint": (28, ("f64",), "f64"), "rintf": (29, ("f32",), "f32"),
    "floorf": (30, ("f32",), "f32"), "f64_to_int": (31, ("f64",), "int"), "f32_to_int": (32, ("f32",), "int"),
}
ELEMENT_TYPE = {"f64": 0, "f32": 1, "int": 2}
N_BULK = 1 << 15
DBL_MAX, DBL_TINY, DBL_MIN = 1.7976931348623157e308, 5e-324, 2.2250738585072014e-308
FLT_MAX = 3.4028234663852886e38
PI = 3.141592653589793
INVPIO2 = 0.6366197723675814   # pm_rem_pio2's own constant


# ---- slots ------------------------------------------------------------------------------------------------------------------------------
def to_slots(a, kind):
    if kind == "f64":
        return np.ascontiguousarray(a, np.float64).view(np.uint64).copy()
    if kind == "f32":
        return np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    if kind == "i64":
        return np.ascontiguousarray(a, np.int64).view(np.uint64).copy()
    assert kind == "u64"
    return np.ascontiguousarray(a, np.uint64).copy()


def from_slots(s, kind):
    if kind == "f64":
        return s.view(np.float64)
    if kind == "f32":
        return s.astype(np.uint32).view(np.float32)
    return s.astype(np.uint32).view(np.int32).astype(np.int64)


def different(a, b, kind):
    """THE comparison rule, on the CPU and on the GPU: two NaNs are equal whatever their sign and payload (those differ between machines:
    aim_canon, att_canon); everything else is compared as raw bits, the sign of zero included -> the indices where a and b differ"""
    if kind == "int":
        return np.nonzero(a != b)[0]
    va, vb = from_slots(a, kind), from_slots(b, kind)
    return np.nonzero((a != b) & ~(np.isnan(va) & np.isnan(vb)))[0]


class Record:
    def __init__(self, name, args):
        self.name, self.func = name, name.split("/")[0]
        self.fid, self.kinds, self.out_kind = FUNCS[self.func]
        self.args = [to_slots(a, k) for a, k in zip(args, self.kinds)]
        assert len(args) == len(self.kinds) and len({len(a) for a in self.args}) == 1, name
        self.edge = name.endswith("/edge")

    def __len__(self):
        return len(self.args[0])

    def values(self, k):
        return from_slots(self.args[k], self.kinds[k]) if self.kinds[k] in ("f64", "f32") else self.args[k]


def write_case_file(path, recs):
    with open(path, "wb") as f:
        f.write(struct.pack("<2I", MAGIC, len(recs)))
        for r in recs:
            f.write(struct.pack("<4IQ", r.fid, ELEMENT_TYPE[r.out_kind], len(r.args), 0, len(r)))
            for a in r.args:
                f.write(a.tobytes())


def read_result_file(path, recs):
    """-> [(device slots | None, host slots)] in the records' order"""
    buf = open(path, "rb").read()
    magic, n, has_device, _ = struct.unpack_from("<4I", buf, 0)
    assert magic == MAGIC and n == len(recs), (magic, n)
    at, out = 16, []
    for r in recs:
        fid, _, count = struct.unpack_from("<2IQ", buf, at)
        assert fid == r.fid and count == len(r), (r.name, fid, count)
        at += 16
        dev = None
        if has_device:
            dev = np.frombuffer(buf, np.uint64, count, at)
            at += 8 * count
        out.append((dev, np.frombuffer(buf, np.uint64, count, at)))
        at += 8 * count
    assert at == len(buf)
    return out


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------
def around(values, k=3, dtype=np.float64):
    """every value with its k neighbours on each side, both signs"""
    out = []
    for v in np.atleast_1d(np.asarray(values, dtype)):
        lo = hi = v
        out.append(v)
        for _ in range(k):
            with np.errstate(over="ignore"):                                  # the neighbour above the largest finite value is infinity
                lo, hi = np.nextafter(lo, dtype(-np.inf)), np.nextafter(hi, dtype(np.inf))
            out += [lo, hi]
    a = np.array(out, dtype)
    return np.concatenate([a, -a])


def log_uniform(rng, n, lo_exp=-1074, hi_exp=1024):
    """magnitudes 2^e with e uniform: every binade of the double range equally often, subnormals included; both signs"""
    v = np.ldexp(rng.uniform(1, 2, n), rng.integers(lo_exp - 1, hi_exp, n))
    v = np.where(np.isfinite(v), v, DBL_MAX)
    return v * rng.choice([-1.0, 1.0], n)


def random_floats(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)


def packet_radians(deg):
    """what att_decode makes of a packet's float: deg * CV_PI / 180.0f"""
    return float(np.float32(deg)) * PI / 180.0


# ---- the functions' cases ---------------------------------------------------------------------------------------------------------------
def _trig():
    rng = np.random.default_rng(101)
    domain = np.concatenate([
        rng.uniform(-7, 7, N_BULK), rng.uniform(-1e4, 1e4, N_BULK),
        around([k * (PI / 4) for k in range(0, 65)]),                        # k pi / 4, |k| <= 64: the reduction's cancellation at its worst
        around([0.7853981633974483, 0.3, 0.78125, 0.6744, float.fromhex("0x1.59428p-1")]),    # the kernels' own cut points
        [0.0, -0.0, DBL_TINY, -DBL_TINY, 2.0 ** -30, -2.0 ** -30, 2.0 ** -27, -2.0 ** -27]])
    edge_n = [2.0 ** 31 - 0.5, 2.0 ** 31 + 0.5, 2.0 ** 31 - 1.0, 2.0 ** 31 - 1.5, 2.0 ** 31]
    edge = np.concatenate([
        log_uniform(rng, 1 << 14),
        around([n * (PI / 2) for n in edge_n] + [n / INVPIO2 for n in edge_n], 8),   # the last quadrant numbers an int holds, and the first it does not
        [math.inf, -math.inf, math.nan, DBL_MAX, -DBL_MAX, 1e10, -1e10, 3.37e9, 3.38e9, -3.37e9, -3.38e9],
        [packet_radians(1e12), packet_radians(-1e12), packet_radians(FLT_MAX), packet_radians(-FLT_MAX)]])
    out = []
    for f in ("sin", "cos", "tan"):
        out += [Record(f + "/domain", [domain]), Record(f + "/edge", [edge])]
    return out


ATAN_BREAKS = [0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** 66, 2.0 ** -28]   # pm_atan's reduction, read off the code


def _atan():
    rng = np.random.default_rng(102)
    x = np.concatenate([log_uniform(rng, N_BULK), rng.uniform(-4, 4, N_BULK), around(ATAN_BREAKS),
                        around([DBL_TINY, DBL_MIN, DBL_MAX, 1.0, 0.5, 1.5]), [0.0, -0.0, math.inf, -math.inf, math.nan]])
    return [Record("atan/domain", [x])]


def _atan2():
    rng = np.random.default_rng(103)
    sp = np.array([0.0, -0.0, 1.0, -1.0, DBL_TINY, -DBL_TINY, DBL_MAX, -DBL_MAX, math.inf, -math.inf, math.nan])
    ys, xs = [np.repeat(sp, len(sp))], [np.tile(sp, len(sp))]
    ys.append(rng.normal(0, 1, N_BULK) * 10.0 ** rng.integers(-3, 3, N_BULK))
    xs.append(rng.normal(0, 1, N_BULK) * 10.0 ** rng.integers(-3, 3, N_BULK))
    ys.append(log_uniform(rng, N_BULK))          # the quotient overflows or underflows
    xs.append(log_uniform(rng, N_BULK))
    q = around(ATAN_BREAKS[:4] + [1.0, 2.0 ** -28])  # the quotient ON a breakpoint: x a power of two, y = q x exactly
    q = np.tile(q[q > 0], 8)
    px = np.ldexp(1.0, rng.integers(-300, 300, len(q))) * rng.choice([-1.0, 1.0], len(q))
    ys.append(q * np.abs(px) * rng.choice([-1.0, 1.0], len(q)))
    xs.append(px)
    return [Record("atan2/domain", [np.concatenate(ys), np.concatenate(xs)])]


LATTICE = np.array([(y, x) for y in range(-64, 65) for x in range(-64, 65)], np.float32)   # what contour points give: 16 641 pairs


def _float_variants():
    rng = np.random.default_rng(104)
    out = [Record("atan2f/lattice", [LATTICE[:, 0], LATTICE[:, 1]]),
           Record("atan2f/bits", [random_floats(rng, 1 << 18), random_floats(rng, 1 << 18)])]
    x = random_floats(rng, 1 << 20)
    x = x[np.abs(x) < 1e4][:1 << 18]
    assert len(x) == 1 << 18
    half_degrees = np.deg2rad(np.arange(-1440, 1441) / 2.0).astype(np.float32)
    for f in ("sinf", "cosf"):
        out += [Record(f + "/bits", [x]), Record(f + "/half_degrees", [half_degrees])]
    return out


def _acos():
    rng = np.random.default_rng(105)
    x = np.concatenate([rng.uniform(-1, 1, N_BULK), around([1.0, 0.5, 0.0, 2.0 ** -57]), 1 - np.geomspace(1e-16, 1e-3, 500), -1 + np.geomspace(1e-16, 1e-3, 500),
                        [1.5, -2.0, 1e300, -math.inf, math.inf, math.nan, -0.0]])
    return [Record("acos/domain", [x])]


def _log():
    rng = np.random.default_rng(106)
    pos = np.abs(log_uniform(rng, N_BULK, -1022, 1024))
    ks = [-1022, -1000, -100, -10, -2, -1, 0, 1, 2, 10, 100, 1000, 1022]
    s2 = around([math.ldexp(1.4142135623730951, k) for k in ks])
    domain = np.concatenate([pos, rng.uniform(0.5, 2, N_BULK), around([1.0], 8)[:17], s2[s2 > 0], np.arange(1, 256) / 255.0])
    # subnormals, zeros, negatives, infinity, NaN: bit moves there, and defined -- the bits must still agree
    outside = np.concatenate([np.abs(log_uniform(rng, 2048, -1074, -1022)), -pos[:2048], [0.0, -0.0, DBL_TINY, -DBL_TINY, math.inf, -math.inf, math.nan]])
    return [Record("log/domain", [domain]), Record("log/outside", [outside])]


LN2 = 0.6931471805599453


def _exp():
    rng = np.random.default_rng(107)
    half = np.array([(j + 0.5) * LN2 for j in range(-1022, 1023)])
    half = np.concatenate([half, np.nextafter(half, -np.inf), np.nextafter(half, np.inf)])
    y = np.concatenate([rng.uniform(-708, 709, N_BULK), rng.uniform(-2, 2, N_BULK), around([708.0, 709.0]), half,
                        [0.0, -0.0, math.inf, -math.inf, math.nan, 1e-300, -1e-300, 750.0, -750.0, DBL_MAX, -DBL_MAX]])
    return [Record("exp/domain", [y])]


@functools.lru_cache(None)
def gammas():
    """(every gamma tests/test_enhance_cpu.py uses, 4096 float gammas uniform in [0, 8])"""
    import test_enhance_cpu as E
    contract = np.array(E.contract_gammas(), np.float32)
    assert len(contract) == E.N_GAMMAS
    return contract, np.random.default_rng(108).uniform(0, 8, 4096).astype(np.float32)


def _pow_lut():
    out = []
    i = np.arange(256)
    for name, g in zip(("contract", "uniform"), gammas()):
        ii, gg = np.tile(i, len(g)), np.repeat(g, 256)
        out.append(Record("pow/" + name, [ii / 255.0, gg.astype(np.float64)]))
        out.append(Record("enh_lut_entry/" + name, [ii, gg]))
    return out


def _enh_gamma():
    import test_enhance_cpu as E
    rng = np.random.default_rng(109)
    cols = [[] for _ in range(6)]
    for n in (1, 64 * 64, 1280 * 1024, 1920 * 1200):
        for hi, lo in E.GAINS:
            s = rng.integers(0, 255 * n + 1, (4096, 3)).astype(np.uint64)
            s = np.concatenate([s, np.zeros((1, 3), np.uint64), np.full((1, 3), 255 * n, np.uint64)])   # ... and the all-0 and all-255 frames
            for k in range(3):
                cols[k].append(s[:, k])
            cols[3].append(np.full(len(s), n, np.int64))
            cols[4].append(np.full(len(s), hi, np.float32))
            cols[5].append(np.full(len(s), lo, np.float32))
    return [Record("enh_gamma/sums", [np.concatenate(c) for c in cols])]


def _hypot():
    import test_pinned_hypot as H   # the generators are that file's: imported, not copied
    (mx, my), (tx, ty) = H.gen_midpoints_and_ties(4000, 500)
    pairs = H.gen_tracker_pairs()
    groups = [H.gen_random_pairs(N_BULK), (mx, my), (tx, ty)] + H.gen_extremes(2000) + [H.ZEROS, H.NON_FINITE, (pairs[:, 0], pairs[:, 1])]
    return [Record("hypot/domain", [np.concatenate([g[0] for g in groups]), np.concatenate([g[1] for g in groups])])]


def _fmod180():
    """ONLY 0 <= x < 720 and NaN: pm_fmod180's loop does not end for +infinity (leaf_funcs.h refuses anything else as well)"""
    rng = np.random.default_rng(110)
    m = np.array([0.0, 180.0, 360.0, 540.0])
    x = np.concatenate([rng.uniform(0, 720, 8192), m, np.nextafter(m, np.inf), np.nextafter(m[1:], -np.inf), [np.nextafter(720.0, 0.0), math.nan]])
    assert ((x >= 0) & (x < 720) | np.isnan(x)).all()
    return [Record("fmod180/domain", [x])]


# ---- the IEEE primitives ------------------------------------------------------------------------------------------------------------------
def _primitives():
    rng = np.random.default_rng(111)
    n = 1 << 14
    f64 = lambda k: rng.integers(0, 1 << 64, k, dtype=np.uint64).view(np.float64)
    sub32 = lambda k: (rng.integers(0, 1 << 23, k, dtype=np.uint64).astype(np.uint32) | (rng.integers(0, 2, k).astype(np.uint32) << 31)).view(np.float32)
    sub64 = lambda k: np.ldexp(rng.integers(0, 1 << 52, k).astype(np.float64), -1074) * rng.choice([-1.0, 1.0], k)
    ints = rng.integers(0, 1 << 26, 2048).astype(np.float64)
    out = [
        Record("sqrt64/cases", [np.concatenate([np.abs(log_uniform(rng, n)), f64(n), ints * ints, around([1.0, 2.0, 4.0, DBL_MIN, DBL_TINY, DBL_MAX]), [0.0, -0.0, math.inf, math.nan]])]),
        Record("sqrt32/cases", [np.concatenate([np.abs(random_floats(rng, n)), random_floats(rng, n), np.abs(sub32(n)), (ints[:1024] * ints[:1024]).astype(np.float32),
                                                around([1.0, 2.0, 4.0, 1.17549435e-38, 1e-45, FLT_MAX], 3, np.float32), np.array([0.0, -0.0, math.inf, math.nan], np.float32)])]),
        Record("div64/cases", [np.concatenate([f64(n), log_uniform(rng, n), sub64(n), rng.uniform(-1, 1, n)]), np.concatenate([f64(n), log_uniform(rng, n), rng.uniform(-4, 4, n), log_uniform(rng, n, 900, 1024)])]),
        Record("div32/cases", [np.concatenate([random_floats(rng, n), sub32(n), rng.uniform(-1, 1, n).astype(np.float32), rng.integers(-64, 65, n).astype(np.float32)]),
                               np.concatenate([random_floats(rng, n), rng.uniform(-4, 4, n).astype(np.float32), (rng.uniform(1, 2, n) * 2.0 ** rng.integers(100, 127, n)).astype(np.float32),
                                               rng.integers(-64, 65, n).astype(np.float32)])]),
    ]
    a, b = log_uniform(rng, n, -400, 400), log_uniform(rng, n, -400, 400)
    c = np.concatenate([-(a[:n // 2] * b[:n // 2]), log_uniform(rng, n // 2, -800, 800)])     # a b + c: the product's own rounding error, and the general case
    out.append(Record("fma64/cases", [np.concatenate([a, f64(n), sub64(n)]), np.concatenate([b, f64(n), rng.uniform(-3, 3, n)]), np.concatenate([c, f64(n), sub64(n)])]))
    tiny32 = (rng.uniform(1, 2, n) * 2.0 ** rng.integers(-90, -50, n)).astype(np.float32) * rng.choice([-1, 1], n).astype(np.float32)
    near32 = (rng.uniform(1, 2, n) * 2.0 ** rng.integers(-128, -120, n)).astype(np.float32)
    out.append(Record("add32/cases", [np.concatenate([sub32(n), sub32(n), near32, random_floats(rng, n)]), np.concatenate([sub32(n), -near32, -near32 * np.float32(1.0000001), random_floats(rng, n)])]))
    out.append(Record("mul32/cases", [np.concatenate([sub32(n), tiny32, near32, random_floats(rng, n)]),
                                      np.concatenate([rng.uniform(-4, 4, n).astype(np.float32), tiny32[::-1], rng.uniform(0, 1, n).astype(np.float32), random_floats(rng, n)])]))
    tiny64 = log_uniform(rng, n, -600, -480)
    near64 = np.abs(log_uniform(rng, n, -1024, -1015))
    out.append(Record("add64/cases", [np.concatenate([sub64(n), sub64(n), near64, f64(n)]), np.concatenate([sub64(n), -near64, -near64 * 1.0000000000001, f64(n)])]))
    out.append(Record("mul64/cases", [np.concatenate([sub64(n), tiny64, near64, f64(n)]), np.concatenate([rng.uniform(-4, 4, n), tiny64[::-1], rng.uniform(0, 1, n), f64(n)])]))
    # narrowing: subnormal floats, exact ties between two floats (and their neighbours in double), the overflow threshold, the general case
    fl = np.concatenate([np.abs(random_floats(rng, n)), np.abs(sub32(n))])
    fl = fl[np.isfinite(fl) & (fl < 3e38)].astype(np.float64)
    ties = (fl + np.nextafter(fl.astype(np.float32), np.float32(np.inf)).astype(np.float64)) * 0.5
    out.append(Record("narrow/cases", [np.concatenate([ties, np.nextafter(ties, 0), np.nextafter(ties, np.inf), -ties, log_uniform(rng, n, -160, -120), log_uniform(rng, n, -200, 200),
                                                       f64(n), around([FLT_MAX, 3.4028235677973366e38, 2.0 ** -149, 2.0 ** -150, 2.0 ** -126]), [0.0, -0.0, math.inf, -math.inf, math.nan]])]))
    k = rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64)
    edges = np.array([(1 << e) + d for e in range(52, 63) for d in (-3, -2, -1, 0, 1, 2, 3)] + [0, 1, -1, (1 << 63) - 1, -(1 << 63), (1 << 63) - 1024, (1 << 63) - 513, (1 << 63) - 512], np.int64)
    out.append(Record("i64_to_f64/cases", [np.concatenate([k, k >> rng.integers(0, 62, n), edges, -edges[:-8]])]))
    u = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    uedges = np.array([(1 << e) + d for e in range(52, 64) for d in (-3, -2, -1, 0, 1, 2, 3)] + [0, 1, (1 << 64) - 1, (1 << 64) - 1024, (1 << 64) - 1025, (1 << 64) - 2048, (1 << 64) - 3072], np.uint64)
    out.append(Record("u64_to_f64/cases", [np.concatenate([u, u >> rng.integers(0, 63, n).astype(np.uint64), uedges])]))
    halves = np.arange(-4096, 4097) * 0.5
    r64 = np.concatenate([rng.uniform(-1e6, 1e6, n), halves, np.nextafter(halves, np.inf), np.nextafter(halves, -np.inf), log_uniform(rng, n), around([2.0 ** 52, 2.0 ** 53, 2.0 ** 51 + 0.5]),
                          [0.0, -0.0, math.inf, -math.inf, math.nan]])
    out.append(Record("rint/cases", [r64]))
    h32 = halves.astype(np.float32)
    r32 = np.concatenate([rng.uniform(-1e6, 1e6, n).astype(np.float32), h32, np.nextafter(h32, np.float32(np.inf)), np.nextafter(h32, np.float32(-np.inf)), random_floats(rng, n),
                          around([2.0 ** 23, 2.0 ** 24, 2.0 ** 22 + 0.5], 3, np.float32), np.array([0.0, -0.0, math.inf, -math.inf, math.nan], np.float32)])
    out += [Record("rintf/cases", [r32]), Record("floorf/cases", [r32])]
    # conversions to int: IN-RANGE arguments only (anything else is undefined in C, which is what the '/edge' records are about)
    d = np.concatenate([rng.uniform(-2147483648.0, 2147483647.0, n), rng.uniform(-300, 300, n), halves, np.nextafter(halves, np.inf), np.nextafter(halves, -np.inf),
                        [0.0, -0.0, 0.999999, -0.999999, 2147483647.0, -2147483648.0, 2147483647.5, -2147483648.5, DBL_TINY, -DBL_TINY]])
    assert (np.trunc(d) >= -2147483648.0).all() and (np.trunc(d) <= 2147483647.0).all()
    out.append(Record("f64_to_int/cases", [d]))
    f = np.concatenate([rng.uniform(-2147483648.0, 2147483520.0, n).astype(np.float32), rng.uniform(-300, 300, n).astype(np.float32), h32,
                        np.array([0.0, -0.0, 0.999999, -0.999999, 2147483520.0, -2147483648.0, 1e-45, -1e-45], np.float32)])
    f = np.clip(f, np.float32(-2147483648.0), np.float32(2147483520.0))
    out.append(Record("f32_to_int/cases", [f]))
    return out


@functools.lru_cache(None)
def records():
    """the whole list, in a fixed order"""
    out = _trig() + _atan() + _atan2() + _float_variants() + _acos() + _log() + _exp() + _pow_lut() + _enh_gamma() + _hypot() + _fmod180() + _primitives()
    assert {r.func for r in out} == set(FUNCS)
    return out


def functions():
    return sorted(FUNCS, key=lambda f: FUNCS[f][0])
