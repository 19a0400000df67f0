"""Inputs of the device probe (tests/devprobe/): numpy only, seeded, shared by tests/test_devprobe_cpu.py and tests/test_devprobe_gpu.py.

case(name) returns, for one function of tests/devprobe/devprobe_fns.h, the rows (uint32 words, the layout of its enum comment) in four groups

    known     known answers and specials: the reference's KAT vectors in both argument orders, the special list of tests/test_math.py,
              arbitrary bit patterns, every float special in every float argument that the function's preconditions admit;
    branch    rows built to force one side of a named branch.  case.branches maps "function.predicate/yes" and ".../no" to row indices.
              The side is decided by a float64 restatement of the predicate with a wide margin wherever the predicate has one; the
              predicates that only rounding can decide (|c0| < FLT_EPS, the a_3 / q clamps, the sorting of n_roots, scale <= FLT_MIN and
              the running maximum before it) are decided by a float32 numpy restatement in the C operation order, which gives the bits
              of the C expression (numpy's float32 + - * / are the IEEE operations, nothing is contracted);
    dense     at least 200 000 rows over the operating range;
    boundary  rows within a few ulps of each decision boundary (no claim which way they go: equality of host and device is the claim).

What a function's precondition excludes is not generated for it (the tests never filter rows):
    m_cbrt_pos, m_pow_pos    x > 0 (no zero, no negative number, no NaN);
    n_point_key              finite input coordinates inside the bounding box, a positive resolution (the caller's checks: a coordinate outside
                             the box or a NaN would reach a float -> unsigned conversion that C leaves undefined);
    a_payload_row            colours in [0, 2^32) (float -> uint32 conversion); the fixture's colours are 0..255;
    a_tc, a_tg, a_edge_weight under EQUALIZATION: |d * bins| < 32768 and no NaN (float -> short conversion);
    plane_normal_wave        count >= 3 (case "normal_cen" holds such rows only);
    edge_weight_quad         colour metric LAB_CIEDE00 (case "a_edge_weight_lab").
"""
import functools
import json
import os

import numpy as np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE = 200000
GROUPS = ("known", "branch", "dense", "boundary")
FN = dict(m_exp=0, m_log=1, m_sin=2, m_cos=3, m_atan2=4, m_cbrt_pos=5, m_pow_pos=6, m_logf=7, m_atan2f=8, m_cosf=9, m_sinf=10,
          n_transform=11, n_point_key=12, n_morton=13, n_plane_normal=14, n_voxel_distance=15, n_rgb2lab=16, n_ciede00=17, n_rgb_eucl=18,
          n_normals_diff=19, n_is_convex=20, n_delta_c_g=21, n_weight_key=22, a_fold=23, a_region_from_acc=24, a_tc=25, a_tg=26,
          a_edge_weight=27, a_edge_weight_lab=27, normal_cen=28, n_ciede00_sq=29)
NI = {0: 4, 1: 4, 2: 4, 3: 4, 4: 4, 5: 4, 6: 4, 7: 4, 8: 4, 9: 4, 10: 4, 11: 4, 12: 11, 13: 4, 14: 13, 15: 22, 16: 3, 17: 6, 18: 6, 19: 12, 20: 12,
      21: 26, 22: 1, 23: 49, 24: 13, 25: 12, 26: 12, 27: 45, 28: 10, 29: 6}
CDF = 8
FOLD_MAX = 8
FLT_MIN = F(1.175494351e-38)
FLT_EPS = F(1.192092896e-07)
# +-0, +- smallest / largest denormal, +-FLT_MIN, +-FLT_MAX, +-inf, NaN
FS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000, 0x7f7fffff, 0xff7fffff,
               0x7f800000, 0xff800000, 0x7fc00000], np.uint32).view(F)
# the special list of tests/test_math.py::test_constants_from_a_table_give_the_same_bits
SPECIAL_D = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 709.78, 709.79, -745.1, -745.3, 1e-310, 5e-324, 2.2250738585072014e-308,
                      1.7976931348623157e308, 2.0 ** 30, -2.0 ** 30, 1.4142135623730951, 0.25, 0.75, 1e300, 1e-300])
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kat.json")))


def words(*cols):
    """Columns (1-D or 2-D; float32 / uint32 / int32 as they are, float64 as two words, low word first) side by side as uint32 rows."""
    out = []
    for c in cols:
        c = np.asarray(c)
        if c.dtype == np.float64:
            c = np.ascontiguousarray(c).view(np.uint32).reshape(c.shape + (2,)).reshape(c.shape[0], -1)
        elif c.dtype in (np.float32, np.int32):
            c = np.ascontiguousarray(c).view(np.uint32)
        elif c.dtype != np.uint32:
            c = c.astype(np.uint32)
        out.append(c.reshape(c.shape[0], -1))
    return np.ascontiguousarray(np.hstack(out))


class Case:
    def __init__(self, name):
        self.name, self.fn, self.ni = name, FN[name], NI[FN[name]]
        self._blocks, self.n = [], 0
        self._groups = {g: [] for g in GROUPS}
        self._branches = {}
        self.expect = {}             # name -> (row indices, expected values): outcomes the CPU test checks on the host probe

    def add(self, rows, group, branch=None):
        rows = np.asarray(rows)
        assert rows.dtype == np.uint32 and rows.ndim == 2 and rows.shape[1] == self.ni, (self.name, rows.dtype, rows.shape, self.ni)
        idx = np.arange(self.n, self.n + len(rows))
        self._blocks.append(rows); self.n += len(rows)
        self._groups[group].append(idx)
        for b in ([branch] if isinstance(branch, str) else (branch or [])):
            self.tag(b, idx)
        return idx

    def tag(self, branch, idx):
        self._branches.setdefault(branch, []).append(np.asarray(idx, np.int64))

    def split(self, name, idx, yes, no=None):
        """idx[yes] -> name/yes, idx[no] -> name/no (no = not yes unless given: rows in neither mask stay untagged)."""
        yes = np.asarray(yes, bool)
        no = ~yes if no is None else np.asarray(no, bool)
        self.tag(name + "/yes", idx[yes]); self.tag(name + "/no", idx[no])

    def finish(self):
        self.rows = np.ascontiguousarray(np.concatenate(self._blocks))
        cat = lambda l: np.concatenate(l) if l else np.zeros(0, np.int64)
        self.groups = {g: cat(v) for g, v in self._groups.items()}
        self.branches = {b: np.unique(cat(v)) for b, v in self._branches.items()}
        del self._blocks
        return self

    def branches_of(self, i):
        return sorted(b for b, v in self.branches.items() if i in v)

    def describe(self, i):
        """Row i for a failure message: its words, as hex floats where they read as floats, and the branches it belongs to."""
        w = self.rows[i]
        if self.fn <= 10:
            d = w.view(np.float64)
            txt = "a = %s, b = %s" % (float(d[0]).hex(), float(d[1]).hex())
        else:
            txt = " ".join("%08x(%s)" % (int(x), float(np.uint32(x).view(F)).hex()) for x in w)
        return "%s row %d: %s; branches %s" % (self.name, i, txt, self.branches_of(i) or "none")


def _ulps32(x, ks):
    """float32 values k ulps away from x for every k of ks (x finite, not zero): shape (len(x) * len(ks),)"""
    b = np.asarray(x, F).view(np.int32).astype(np.int64)
    k = np.asarray(ks, np.int64)
    step = np.where(b[:, None] < 0, -k[None, :], k[None, :])         # negative floats grow with a decreasing bit pattern
    return (b[:, None] + step).astype(np.int32).view(F).reshape(-1)


def _ulps64(x, ks):
    b = np.asarray(x, np.float64).view(np.int64)
    k = np.asarray(ks, np.int64)
    step = np.where(b[:, None] < 0, -k[None, :], k[None, :])
    return (b[:, None] + step).view(np.float64).reshape(-1)


KS = np.arange(-4, 5)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _with_specials(base, cols):
    """base (one float32 row) repeated with each float special in each column of cols, then with the special in all of them"""
    base = np.asarray(base, F)
    rows = []
    for s in FS:
        for c in cols:
            r = base.copy(); r[c] = s; rows.append(r)
        r = base.copy(); r[list(cols)] = s; rows.append(r)
    return np.array(rows, F)


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 restatements (also the plain references of tests/test_devprobe_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def lab_f64(rgb):
    """sRGB (D65) -> CIE L*a*b* in float64 (the formula of tests/test_pins.py, vectorised); also returns (v, X, Y, Z) for the branch predicates"""
    v = np.asarray(rgb, np.float64) / 255.0
    with np.errstate(all="ignore"):
        c = np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
        X = (c[:, 0] * 0.412453 + c[:, 1] * 0.357580 + c[:, 2] * 0.180423) / 0.950456
        Y = c[:, 0] * 0.212671 + c[:, 1] * 0.715160 + c[:, 2] * 0.072169
        Z = (c[:, 0] * 0.019334 + c[:, 1] * 0.119193 + c[:, 2] * 0.950227) / 1.088754
        f = lambda t: np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16.0 / 116.0)
        L = np.where(Y > 0.008856, 116.0 * f(Y) - 16.0, 903.3 * Y)
        lab = np.stack([L, 500.0 * (f(X) - f(Y)), 200.0 * (f(Y) - f(Z))], 1)
    return lab, (v, X, Y, Z)


def _lab_default(rgb):
    return lab_f64(rgb)[0].astype(F)


def ciede2000_f64(lab1, lab2):
    """CIEDE2000 (Sharma, Wu, Dalal 2005, kL = kC = kH = 1) in float64 on float32 Lab inputs, in degrees as the paper states it.
    Returns (dE, parts) with the intermediates the branch bookkeeping needs."""
    l1 = np.asarray(lab1, F).astype(np.float64); l2 = np.asarray(lab2, F).astype(np.float64)
    L1, a1, b1 = l1.T; L2, a2, b2 = l2.T
    with np.errstate(all="ignore"):
        C1 = np.hypot(a1, b1); C2 = np.hypot(a2, b2)
        Cb7 = ((C1 + C2) / 2.0) ** 7
        G = 0.5 * (1.0 - np.sqrt(Cb7 / (Cb7 + 25.0 ** 7)))
        ap1 = (1.0 + G) * a1; ap2 = (1.0 + G) * a2
        Cp1 = np.hypot(ap1, b1); Cp2 = np.hypot(ap2, b2)
        h1 = np.where((ap1 == 0) & (b1 == 0), 0.0, np.degrees(np.arctan2(b1, ap1)) % 360.0)
        h2 = np.where((ap2 == 0) & (b2 == 0), 0.0, np.degrees(np.arctan2(b2, ap2)) % 360.0)
        grey = Cp1 * Cp2 == 0
        dh = h2 - h1
        dhp = np.where(grey, 0.0, np.where(dh > 180.0, dh - 360.0, np.where(dh < -180.0, dh + 360.0, dh)))
        dLp = L2 - L1; dCp = Cp2 - Cp1
        dHp = 2.0 * np.sqrt(Cp1 * Cp2) * np.sin(np.radians(dhp / 2.0))
        Lb = (L1 + L2) / 2.0; Cb = (Cp1 + Cp2) / 2.0
        hs = h1 + h2
        hb = np.where(grey, hs, np.where(np.abs(h1 - h2) <= 180.0, hs / 2.0, np.where(hs < 360.0, (hs + 360.0) / 2.0, (hs - 360.0) / 2.0)))
        T = 1.0 - 0.17 * np.cos(np.radians(hb - 30.0)) + 0.24 * np.cos(np.radians(2.0 * hb)) + 0.32 * np.cos(np.radians(3.0 * hb + 6.0)) \
            - 0.20 * np.cos(np.radians(4.0 * hb - 63.0))
        dth = 30.0 * np.exp(-(((hb - 275.0) / 25.0) ** 2))
        Rc = 2.0 * np.sqrt(Cb ** 7 / (Cb ** 7 + 25.0 ** 7))
        Sl = 1.0 + 0.015 * (Lb - 50.0) ** 2 / np.sqrt(20.0 + (Lb - 50.0) ** 2)
        Sc = 1.0 + 0.045 * Cb; Sh = 1.0 + 0.015 * Cb * T
        Rt = -np.sin(np.radians(2.0 * dth)) * Rc
        tL, tC, tH = dLp / Sl, dCp / Sc, dHp / Sh
        dE = np.sqrt(tL * tL + tC * tC + tH * tH + Rt * tC * tH)
    return dE, dict(h1=h1, h2=h2, dh=dh, grey=grey, tL=tL, tC=tC, hs=hs, chroma1=(ap1 == 0) & (b1 == 0), chroma2=(ap2 == 0) & (b2 == 0))


def voxel_distance_f64(rows):
    """n_voxel_distance in float64 on the float32 words of DP_VOXEL_DISTANCE rows"""
    f = rows.view(F).astype(np.float64)
    c, v = f[:, 0:9], f[:, 9:18]
    with np.errstate(all="ignore"):
        spatial = np.sqrt(((c[:, 0:3] - v[:, 0:3]) ** 2).sum(1)) / f[:, 18]
        color = np.sqrt(((c[:, 3:6] - v[:, 3:6]) ** 2).sum(1)) / 255.0
        cosn = 1.0 - np.abs((c[:, 6:9] * v[:, 6:9]).sum(1))
        return cosn * f[:, 19] + color * f[:, 20] + spatial * f[:, 21]


def morton_py(x, y, z, depth):
    """bit b of x, y, z -> bits 3b + 2, 3b + 1, 3b for b < depth, by a plain loop over the bits (uint64 arrays)"""
    x, y, z = (np.asarray(v, np.uint64) for v in (x, y, z))
    depth = np.asarray(depth, np.uint64)
    c = np.zeros(len(x), np.uint64)
    for b in range(21):
        on = np.uint64(b) < depth
        for v, s in ((x, 2), (y, 1), (z, 0)):
            c |= np.where(on, ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + s), np.uint64(0))
    return c


def grid_f64(mn, mx, res):
    """n_grid_from_bbox / n_key_bit_size in float64 numpy (the same IEEE operations; libm's log in place of m_log, which the - eps in the
    source makes immaterial away from depth borders).  Returns (min after centring, depth)."""
    lo = np.minimum(mn, mx).astype(np.float64); hi = np.maximum(mn, mx).astype(np.float64)
    r = np.asarray(res, F).astype(np.float64)
    eps = float(FLT_EPS)
    k = np.ceil((hi - lo - eps) / r[:, None]).max(1)
    k = np.maximum(k, 2.0)
    d = np.ceil(np.log(k) / np.log(2.0) - eps)
    side = (2.0 ** d) * r
    over = (side[:, None] - (hi - lo)) / 2.0
    return np.where(over > eps, lo - over, lo), d.astype(np.int64), over


# ---------------------------------------------------------------------------------------------------------------------------------
# f3ds_math.h
# ---------------------------------------------------------------------------------------------------------------------------------
def _case_math(name):
    fn = FN[name]
    rng = np.random.default_rng(1000 + fn)
    c = Case(name)
    base = fn if fn < 7 else {7: 1, 8: 4, 9: 3, 10: 2}[fn]
    pos = base in (5, 6)
    two = base in (4, 6)

    def put(a, b, group, branch=None):
        a = np.asarray(a, np.float64); b = np.broadcast_to(np.asarray(b, np.float64), a.shape)
        if pos:
            a = np.abs(a); keep = a > 0
            a, b = a[keep], b[keep]
        return c.add(words(a, b), group, branch), a, b

    fs = FS.astype(np.float64)
    bits = rng.integers(0, 2 ** 64, 20000, dtype=np.uint64).view(np.float64)
    sp = np.concatenate([SPECIAL_D, fs])
    put(sp, sp[::-1], "known")
    put(np.repeat(sp, len(sp)), np.tile(sp, len(sp)), "known")
    put(bits, bits[::-1], "known")
    put(np.concatenate([SPECIAL_D, fs]), 2.4, "known")
    n = DENSE
    if base == 0:
        put(rng.uniform(-200, 50, n), 0.0, "dense")
        idx, a, _ = put(np.concatenate([rng.uniform(-1000, -750, 16), rng.uniform(-740, 700, 16)]), 0.0, "branch"); c.split("m_exp.underflow", idx, a < -745.2)
        idx, a, _ = put(np.concatenate([rng.uniform(710, 1000, 16), rng.uniform(-740, 709, 16)]), 0.0, "branch"); c.split("m_exp.overflow", idx, a > 709.79)
        k = np.arange(-1070, 1025, 7)
        put(np.concatenate([_ulps64([-745.2, 709.782712893384], KS), _ulps64((k + 0.5) * np.log(2.0), KS)]), 0.0, "boundary")
    elif base == 1:
        x = np.exp(rng.uniform(-40, 40, n)) if fn == 1 else rng.uniform(0.3, 12.0, n).astype(F).astype(np.float64)
        put(x, 0.0, "dense")
        idx, a, _ = put(np.concatenate([rng.uniform(1e-320, 2e-308, 16), np.exp(rng.uniform(-40, 40, 16))]), 0.0, "branch"); c.split("m_log.subnormal", idx, a < 2.2250738585072014e-308)
        idx, a, _ = put(np.concatenate([-np.exp(rng.uniform(-40, 40, 12)), np.zeros(4), np.exp(rng.uniform(-40, 40, 16))]), 0.0, "branch"); c.split("m_log.not_positive", idx, ~(a > 0))
        m = np.concatenate([rng.uniform(1.45, 1.99, 16), rng.uniform(1.01, 1.40, 16)]) * 2.0 ** rng.integers(-30, 30, 32)
        idx, a, _ = put(m, 0.0, "branch"); c.split("m_log.mantissa>sqrt2", idx, np.frexp(a)[0] * 2 > 1.4142135623730951)
        put(np.concatenate([_ulps64(1.4142135623730951 * 2.0 ** np.arange(-60, 60, 3), KS), _ulps64([2.2250738585072014e-308, 1.0], KS),
                            _ulps32(np.array([1.0, 1.4142135, 2.0, 0.5], F), KS).astype(np.float64)]), 0.0, "boundary")
    elif base in (2, 3):
        x = rng.uniform(-30, 30, n) if fn < 7 else rng.uniform(0, np.pi / 3, n).astype(F).astype(np.float64)
        put(x, 0.0, "dense")
        q = np.repeat(np.arange(-8, 9), 4)
        idx, a, _ = put((q + rng.uniform(-0.4, 0.4, len(q))) * (np.pi / 2), 0.0, "branch")
        c.split(name + ".quadrant&1", idx, (q & 1) != 0); c.split(name + ".quadrant&2", idx, (((q + (1 if base == 3 else 0)) & 2) != 0))
        idx, a, _ = put(np.concatenate([rng.uniform(2.0 ** 30, 2.0 ** 40, 8), -rng.uniform(2.0 ** 30, 2.0 ** 40, 8), rng.uniform(-1e5, 1e5, 16)]), 0.0, "branch")
        c.split(name + ".out_of_range", idx, ~(np.abs(a) < 2.0 ** 30))
        k = np.arange(-40, 41)
        put(np.concatenate([_ulps64((k + 0.5) * (np.pi / 2), KS), _ulps64(k[k != 0] * (np.pi / 2), KS), _ulps64([2.0 ** 30, -2.0 ** 30], KS)]), 0.0, "boundary")
    elif base == 4:
        y, x = rng.uniform(-100, 100, n), rng.uniform(-100, 100, n)
        if fn == 8:
            y, x = y.astype(F).astype(np.float64), x.astype(F).astype(np.float64)
        put(y, x, "dense")
        t = np.concatenate([rng.uniform(0.01, 0.2, 16), rng.uniform(0.3, 0.7, 16), rng.uniform(0.8, 0.99, 16)])
        big = rng.uniform(0.5, 50, len(t)); sx = rng.choice([-1.0, 1.0], len(t)); sy = rng.choice([-1.0, 1.0], len(t))
        idx, a, b = put(sy * t * big, sx * big, "branch")           # |y| < |x|
        c.split("m_atan2.steep", idx, np.zeros(len(t), bool)); c.split("m_atan01.t<0.25", idx, t < 0.25); c.split("m_atan01.t<0.75", idx, t < 0.75)
        c.split("m_atan2.x<0", idx, sx < 0)
        idx, a, b = put(sy * big, sx * t * big, "branch")           # |y| > |x|
        c.split("m_atan2.steep", idx, np.ones(len(t), bool)); c.split("m_atan2.x<0", idx, sx < 0)
        z = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.3, -2.5e3, 7e-200])
        idx, a, b = put(np.repeat(z, len(z)), np.tile(z, len(z)), "branch")
        c.split("m_atan2.special", idx, ~((np.abs(a) > 0) & (np.abs(b) > 0) & np.isfinite(a) & np.isfinite(b)))
        r = _ulps64([0.25, 0.75, 1.0], KS)
        s = np.array([[1, 1], [1, -1], [-1, 1], [-1, -1]], np.float64)
        put(np.concatenate([r * sy_ for sy_, _ in s] + [np.ones(len(r)) * sy_ for sy_, _ in s]),
            np.concatenate([np.ones(len(r)) * sx_ for _, sx_ in s] + [r * sx_ for _, sx_ in s]), "boundary")
    elif base == 5:
        put(np.exp(rng.uniform(-20, 5, n)), 0.0, "dense")
        put(_ulps64(np.concatenate([[float(F(0.008856)), 1.0, 8.0, 0.125], F(rng.uniform(0, 1.1, 200)).astype(np.float64)]), KS), 0.0, "boundary")
    elif base == 6:
        put(rng.uniform(0.05, 1.0, n).astype(F).astype(np.float64), 2.4, "dense")
        put(np.exp(rng.uniform(-20, 5, 20000)), rng.uniform(-3, 3, 20000), "dense")
        put(_ulps64([(0.04045 + 0.055) / 1.055, 1.0, float(F(0.055) / F(1.055))], KS), 2.4, "boundary")
    return c.finish()


# ---------------------------------------------------------------------------------------------------------------------------------
# grid: n_transform, n_grid_from_bbox + n_point_key, n_morton
# ---------------------------------------------------------------------------------------------------------------------------------
def _case_transform():
    rng = np.random.default_rng(11)
    c = Case("n_transform")
    for use in (0, 1):
        s = _with_specials([0.5, -0.3, 2.0], [0, 1, 2])
        c.add(words(s, np.full(len(s), use, np.uint32)), "known")
    xyz = np.stack([rng.uniform(-5, 5, 32), rng.uniform(-5, 5, 32), rng.uniform(0.3, 12, 32)], 1).astype(F)
    use = np.repeat([1, 0], 16).astype(np.uint32)
    c.split("n_transform.use_transform", c.add(words(xyz, use), "branch"), use == 1)
    n = DENSE
    xyz = np.stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(0.3, 12, n)], 1).astype(F)
    c.add(words(xyz, (rng.random(n) < 0.75).astype(np.uint32)), "dense")
    z = np.concatenate([_ulps32(F(1.4142135) * F(2.0) ** np.arange(-6, 6).astype(F), KS), _ulps32(np.array([1.0, 0.5, 2.0], F), KS), FS[2:8]])
    c.add(words(np.stack([np.full(len(z), 0.7, F), np.full(len(z), -1.3, F), z], 1), np.ones(len(z), np.uint32)), "boundary")
    return c.finish()


def _case_point_key():
    rng = np.random.default_rng(12)
    c = Case("n_point_key")
    row = lambda mn, mx, res, p, use: words(np.asarray(mn, F), np.asarray(mx, F), np.asarray(res, F), np.asarray(p, F), np.asarray(use, np.uint32))
    ones = lambda n, v: np.full((n, 3), v, F)

    # cell borders on grids that n_key_bit_size leaves where they are (the box is exactly 2^depth cells): coordinate min + k * res
    # is a float, so the key on the border is k, one ulp below it k - 1, one ulp above it k
    on, below, above = [], [], []
    for res, lo, depth in ((F(2.0) ** -7, F(-1.0), 8), (F(2.0) ** -7, F(0.0), 10), (F(0.008), F(0.0), 8), (F(0.02), F(0.0), 11)):
        span = F(float(res) * 2.0 ** depth)
        assert float(span) == float(res) * 2.0 ** depth
        ks = np.unique(np.concatenate([2 ** np.arange(0, depth), [2 ** depth - 1] if float(res) == 2.0 ** -7 else [], rng.integers(1, 2 ** depth, 24) if float(res) == 2.0 ** -7 else []]).astype(np.int64))
        for k in ks:
            p = float(lo) + k * float(res)
            assert float(F(p)) == p
            kk = np.array([k, ks[(k * 7) % len(ks)], ks[(k * 13) % len(ks)]])          # another border cell on the other two axes
            pp = (float(lo) + kk * float(res)).astype(F)
            if (pp == 0).any():          # (one ulp below zero is a denormal: min + it rounds back to the border in float64)
                continue
            for dst, q, e in ((on, pp, kk), (below, np.nextafter(pp, F(-np.inf)), kk - 1), (above, np.nextafter(pp, F(np.inf)), kk)):
                dst.append((ones(1, lo)[0], ones(1, lo)[0] + span, res, q, e))
    for nm, lst in (("on", on), ("below", below), ("above", above)):
        mn = np.array([t[0] for t in lst]); mx = np.array([t[1] for t in lst]); res = np.array([t[2] for t in lst]); p = np.array([t[3] for t in lst])
        idx = c.add(row(mn, mx, res, p, np.zeros(len(lst))), "branch", ["n_point_key.division_path/yes", "n_key_bit_size.over>eps/no", "n_point_key.use_transform/no"])
        c.expect["border_" + nm] = (idx, np.array([t[4] for t in lst], np.uint32))

    def generic(n, use, rng):
        """boxes of a depth camera's frame with one point inside each; use: the box lies around the transformed point"""
        res = rng.choice(np.array([0.008, 0.02, 0.005, 0.01], F), n)
        if use:
            raw = np.stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(0.3, 12, n)], 1).astype(F)
            t = np.stack([raw[:, 0].astype(np.float64) / raw[:, 2], raw[:, 1].astype(np.float64) / raw[:, 2], np.log(raw[:, 2].astype(np.float64))], 1)
            mn = (t - rng.uniform(0.01, 2.0, (n, 3))).astype(F); mx = (t + rng.uniform(0.01, 2.0, (n, 3))).astype(F)
            return mn, mx, res, raw
        mn = rng.uniform(-3, 0, (n, 3)).astype(F); mx = (mn + rng.uniform(0.5, 4.0, (n, 3))).astype(F)
        p = np.clip((mn + rng.random((n, 3)) * (mx - mn)).astype(F), mn, mx)
        return mn, mx, res, p

    for use in (0, 1):
        mn, mx, res, p = generic(DENSE // 2, use, rng)
        c.add(row(mn, mx, res, p, np.full(len(p), use)), "dense")
    # mid-cell points (fast path), and the other branches
    mn, mx, res, _ = generic(256, 0, rng)
    gmin, depth, over = grid_f64(mn, mx, res)
    k = np.floor(rng.random((256, 3)) * ((mx.astype(np.float64) - gmin) / res[:, None].astype(np.float64) - 2)) + 1
    p = (gmin + (k + 0.5) * res[:, None].astype(np.float64)).astype(F)
    ok = ((p >= mn) & (p <= mx)).all(1)
    idx = c.add(row(mn[ok], mx[ok], res[ok], p[ok], np.zeros(ok.sum())), "known", ["n_point_key.division_path/no", "n_grid_from_bbox.lo<hi/yes", "n_key_bit_size.depth_error/no", "n_key_bit_size.k>2/yes"])
    c.tag("n_key_bit_size.over>eps/yes", idx[(over[ok] > 1e-3).all(1)])
    c.expect["mid_cell"] = (idx, k[ok].astype(np.uint32))
    mn, mx, res, p = generic(32, 1, rng)
    idx = c.add(row(mn, mx, res, p, np.ones(32)), "branch", ["n_point_key.use_transform/yes", "n_point_key.transformed_finite/yes"])
    bad = p.copy(); bad[:16, 2] = 0.0; bad[16:, 2] = -bad[16:, 2]                       # z = 0: x / z infinite; z < 0: log(z) NaN
    idx = c.add(row(mn, mx, res, bad, np.ones(32)), "branch", "n_point_key.transformed_finite/no")
    c.expect["key_zero"] = (idx, np.zeros((32, 3), np.uint32))
    mn, mx, res, p = generic(32, 0, rng)
    c.add(row(mx, mn, res, p, np.zeros(32)), "branch", "n_grid_from_bbox.lo<hi/no")            # corners swapped
    c.add(row(mn, mn + F(100.0), np.full(32, 1e-5, F), p, np.zeros(32)), "branch", "n_key_bit_size.depth_error/yes")
    tiny = (mn + rng.uniform(0.2, 1.5, (32, 3)).astype(F) * res[:, None]).astype(F)
    c.add(row(mn, tiny, res, mn, np.zeros(32)), "branch", "n_key_bit_size.k>2/no")
    # a few ulps around the borders of generic grids (their minimum moved by the centring)
    mn, mx, res, _ = generic(2000, 0, rng)
    gmin, depth, over = grid_f64(mn, mx, res)
    k = np.floor(rng.random((2000, 3)) * ((mx.astype(np.float64) - gmin) / res[:, None].astype(np.float64) - 2)) + 1
    p0 = (gmin + k * res[:, None].astype(np.float64)).astype(F)
    for j in KS:
        p = (p0.view(np.int32) + np.where(p0 < 0, -j, j).astype(np.int32)).view(F)
        ok = ((p >= mn) & (p <= mx)).all(1) & (p0 != 0).all(1)
        c.add(row(mn[ok], mx[ok], res[ok], p[ok], np.zeros(ok.sum())), "boundary")
    return c.finish()


def _case_morton():
    rng = np.random.default_rng(13)
    c = Case("n_morton")
    full = 2 ** 21 - 1
    rows = [[0, 0, 0, 21], [full, full, full, 21], [full, 0, 0, 21], [0, full, 0, 21], [0, 0, full, 21], [full, full, full, 10], [full, full, full, 0]]
    for b in range(21):
        for a in range(3):
            k = [0, 0, 0]; k[a] = 1 << b
            rows += [k + [21], k + [b + 1], k + [b]]
    c.add(np.array(rows, np.uint32), "known")
    d = np.repeat(np.arange(0, 22), 16).astype(np.uint32)
    k = rng.integers(0, 2 ** 21, (len(d), 3)).astype(np.uint32)
    c.split("n_morton.depth<=10", c.add(words(k, d), "branch"), d <= 10)
    n = DENSE
    d = rng.integers(1, 22, n).astype(np.uint32)
    k = rng.integers(0, 2 ** 21, (n, 3)).astype(np.uint32)
    k[: n // 2] &= ((1 << d[: n // 2, None]) - 1).astype(np.uint32)
    c.add(words(k, d), "dense")
    e = np.array([2 ** 10 - 1, 2 ** 10, 2 ** 10 + 1, 2 ** 11 - 1, 2 ** 20, full], np.uint32)
    g = np.array([[x, y, z, dd] for x in e for y in e[:3] for z in e[3:] for dd in (9, 10, 11, 12, 20, 21)], np.uint32)
    c.add(g, "boundary")
    return c.finish()


# ---------------------------------------------------------------------------------------------------------------------------------
# plane normals: point sets -> the nine running sums (float32, in list order, as the device's ordered fold and tests/emul have them)
# ---------------------------------------------------------------------------------------------------------------------------------
def sums_f32(pts):
    """pts (m, k, 3) float32 -> (m, 9) float32 sums xx xy xz yy yz zz x y z accumulated point after point"""
    pts = np.asarray(pts, F)
    acc = np.zeros((pts.shape[0], 9), F)
    with np.errstate(all="ignore"):
        for i in range(pts.shape[1]):
            x, y, z = pts[:, i, 0], pts[:, i, 1], pts[:, i, 2]
            for j, t in enumerate((x * x, x * y, x * z, y * y, y * z, z * z, x, y, z)):
                acc[:, j] += t
    return acc


def _patches(rng, m, k, transform=False, lo=0.3, hi=12.0):
    """m planar patches of k points of voxel-neighbourhood size (tests/test_pins.py::_patch, vectorised) 0.3 - 12 m from the origin;
    transform: the coordinates after the single-camera transform (x / z, y / z, log z)"""
    nrm = _unit(rng.normal(0, 1, (m, 3)))
    u = _unit(np.cross(nrm, [1.0, 0.3, 0.2])); v = np.cross(nrm, u)
    centre = _unit(rng.normal(0, 1, (m, 3))) * rng.uniform(lo, hi, (m, 1))
    if transform:
        centre[:, 2] = np.abs(centre[:, 2]) + 0.3
    ext = rng.uniform(0.01, 0.05, (m, 2))
    noise = rng.uniform(0.0, 0.05, (m, 1)) * ext.min(1, keepdims=True)
    pts = centre[:, None, :] + (rng.uniform(-1, 1, (m, k, 1)) * ext[:, None, 0:1]) * u[:, None, :] + (rng.uniform(-1, 1, (m, k, 1)) * ext[:, None, 1:2]) * v[:, None, :] \
        + (rng.normal(0, 1, (m, k, 1)) * noise[:, None, :]) * nrm[:, None, :]
    if transform:
        z = np.maximum(pts[:, :, 2], 0.2)
        pts = np.stack([pts[:, :, 0] / z, pts[:, :, 1] / z, np.log(z)], 2)
    return pts.astype(F)


DENSE_SIZES = ((3, 40000), (4, 31000), (5, 25000), (8, 25000), (13, 25000), (25, 25000), (40, 15000), (100, 10000), (300, 3000), (757, 1000))


@functools.lru_cache(maxsize=None)
def _dense_sums():
    """(acc (n, 9), count (n,), first point (n, 3)) of random patches of 3 - 757 points, every other block after the transform"""
    rng = np.random.default_rng(14)
    acc, cnt, first = [], [], []
    for b, (k, m) in enumerate(DENSE_SIZES):
        for lo in range(0, m, 5000):
            p = _patches(rng, min(5000, m - lo), k, transform=(b % 2 == 1))
            acc.append(sums_f32(p)); cnt.append(np.full(len(p), k, np.uint32)); first.append(p[:, 0, :])
    return np.concatenate(acc), np.concatenate(cnt), np.concatenate(first)


def neighbourhood_sums(xyz, nbr):
    """sums over the one-ring of every voxel (oracle debug arrays VOXEL_XYZ (V, 3), VOXEL_NEIGHBORS (V, 27), -1 = none)"""
    xyz = np.asarray(xyz, F).reshape(-1, 3); nbr = np.asarray(nbr, np.int32).reshape(-1, 27)
    acc = np.zeros((len(xyz), 9), F)
    for s in range(27):
        ok = nbr[:, s] >= 0
        q = xyz[np.where(ok, nbr[:, s], 0)]
        x, y, z = q[:, 0], q[:, 1], q[:, 2]
        for j, t in enumerate((x * x, x * y, x * z, y * y, y * z, z * z, x, y, z)):
            acc[:, j] += np.where(ok, t, F(0))
    return acc, (nbr >= 0).sum(1).astype(np.uint32)


def normal_predicates(acc, count):
    """The decisions of n_plane_normal / n_roots up to the sorted roots as float32 numpy in the C operation order (bit for bit the C
    expressions up to the trigonometric step; from there float64 libm rounded to float32, which the rare last-bit difference of
    m_atan2f / m_cosf / m_sinf can only move on a tie).  Returns {predicate: bool array}; meaningful where count >= 3."""
    a = np.asarray(acc, F); cnt = np.asarray(count).astype(F)
    P = {}
    with np.errstate(all="ignore"):
        a = a / cnt[:, None]
        c00 = a[:, 0] - a[:, 6] * a[:, 6]; c01 = a[:, 1] - a[:, 6] * a[:, 7]; c02 = a[:, 2] - a[:, 6] * a[:, 8]
        c11 = a[:, 3] - a[:, 7] * a[:, 7]; c12 = a[:, 4] - a[:, 7] * a[:, 8]; c22 = a[:, 5] - a[:, 8] * a[:, 8]
        scale = np.abs(c00)
        for nm, t in (("c01", c01), ("c02", c02), ("c11", c11), ("c12", c12), ("c22", c22)):
            up = np.abs(t) > scale
            P["n_plane_normal.|%s|>scale" % nm] = up
            scale = np.where(up, np.abs(t), scale)
        tiny = scale <= FLT_MIN
        P["n_plane_normal.scale<=FLT_MIN"] = tiny
        scale = np.where(tiny, F(1), scale)
        m00, m01, m02, m11, m12, m22 = (t / scale for t in (c00, c01, c02, c11, c12, c22))
        c0 = m00 * m11 * m22 + F(2) * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01
        c1 = m00 * m11 - m01 * m01 + m00 * m22 - m02 * m02 + m11 * m22 - m12 * m12
        c2 = m00 + m11 + m22
        small = np.abs(c0) < FLT_EPS
        P["n_roots.|c0|<eps"] = small
        inv3 = F(1.0 / 3.0); sqrt3 = F(1.7320508075688772)
        c2_3 = c2 * inv3
        a_3 = (c1 - c2 * c2_3) * inv3
        P["n_roots.a_3>0"] = (a_3 > 0) & ~small
        a_3 = np.where(a_3 > 0, F(0), a_3)
        half_b = F(0.5) * (c0 + c2_3 * (F(2) * c2_3 * c2_3 - c1))
        q = half_b * half_b + a_3 * a_3 * a_3
        P["n_roots.q>0"] = (q > 0) & ~small
        q = np.where(q > 0, F(0), q)
        rho = np.sqrt(-a_3)
        theta = np.arctan2(np.sqrt(-q).astype(np.float64), half_b.astype(np.float64)).astype(F) * inv3
        ct = np.cos(theta.astype(np.float64)).astype(F); st = np.sin(theta.astype(np.float64)).astype(F)
        r0 = c2_3 + F(2) * rho * ct; r1 = c2_3 - rho * (ct + sqrt3 * st); r2 = c2_3 - rho * (ct - sqrt3 * st)
        s1 = r0 >= r1
        r0, r1 = np.where(s1, r1, r0), np.where(s1, r0, r1)
        s2 = r1 >= r2
        r1, r2 = np.where(s2, r2, r1), np.where(s2, r1, r2)
        s3 = s2 & (r0 >= r1)
        r0 = np.where(s3, r1, r0)
        P["n_roots.swap r0>=r1"] = s1 & ~small; P["n_roots.swap r1>=r2"] = s2 & ~small; P["n_roots.swap r0>=r1 again"] = s3 & ~small
        neg = (r0 <= 0) & ~small
        P["n_roots.r[0]<=0"] = neg
        d = (c2 * c2).astype(np.float64) - 4.0 * c1.astype(np.float64)
        P["n_roots2.d<0"] = (d.astype(F) < 0) & (small | neg)
        P["_cubic"] = ~small; P["_roots2"] = small | neg
    return P


# predicates that only exist on one path: their "no" side is counted among the rows of that path
_PRED_DOMAIN = {"n_roots.a_3>0": "_cubic", "n_roots.q>0": "_cubic", "n_roots.swap r0>=r1": "_cubic", "n_roots.swap r1>=r2": "_cubic",
                "n_roots.swap r0>=r1 again": "_cubic", "n_roots.r[0]<=0": "_cubic", "n_roots2.d<0": "_roots2"}


@functools.lru_cache(maxsize=None)
def _branch_sets():
    """Point sets that force the branches of n_plane_normal: (acc, count, first point, {tag: local indices}, expectations)"""
    rng = np.random.default_rng(15)
    acc, cnt, first, tags, n = [], [], [], {}, [0]

    def put(pts, tag=None, count=None):
        pts = np.asarray(pts, F)
        a = sums_f32(pts)
        k = np.full(len(pts), pts.shape[1], np.uint32) if count is None else np.asarray(count, np.uint32)
        idx = np.arange(n[0], n[0] + len(pts)); n[0] += len(pts)
        acc.append(a); cnt.append(k); first.append(pts[:, 0, :] if pts.shape[1] else np.zeros((len(pts), 3), F))
        for t in ([tag] if isinstance(tag, str) else (tag or [])):
            tags.setdefault(t, []).append(idx)
        return idx

    grid = lambda m, k: rng.integers(-8, 9, (m, k)).astype(np.float64) / 8.0           # coordinates that are exact in float32, and so are their sums
    for axis, tag in ((2, "plane_z"), (1, "plane_y"), (0, "plane_x")):              # exactly coplanar: one coordinate constant (a power of two)
        for k in (3, 4, 12, 40):
            p = np.stack([grid(8, k), grid(8, k), grid(8, k)], 2)
            o1, o2 = (axis + 1) % 3, (axis + 2) % 3
            p[:, 0, [o1, o2]] = [0, 0]; p[:, 1, [o1, o2]] = [1, 0]; p[:, 2, [o1, o2]] = [0, 1]      # three points that span the plane
            p[:, :, axis] = rng.choice([0.5, 1.0, 2.0, -1.0], (8, 1))
            put(p, tag)
    for k in (3, 5, 20):                                                           # collinear along an axis, and along a diagonal
        t = grid(8, k); t[:, 0] = 0; t[:, 1] = 1
        put(np.stack([t, np.full_like(t, 0.5), np.full_like(t, 1.0)], 2), "collinear")
        put(np.stack([t, t, t], 2) + 0.25, "collinear")
    for k in (3, 7, 30):                                                           # coincident
        put(np.tile(np.array([1.0, 2.0, 4.0]), (8, k, 1)), "coincident")
        put(np.tile(rng.uniform(-3, 3, (8, 1, 3)), (1, k, 1)), "coincident_generic")
    put(_patches(rng, 64, 3), "three_points")
    for k in (0, 1, 2):
        put(_patches(rng, 16, 2)[:, :k, :], "count<3")
    p = _patches(rng, 16, 9); p[:, 4, 1] = np.nan; put(p, "nan_in_sums")
    p = _patches(rng, 16, 9); p[:, 2, 0] = np.inf; put(p, "nan_in_sums")
    # equal or nearly equal eigenvalues: the a_3 / q clamps and the orderings of the roots are rounding decisions there
    octa = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    cube = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    for shape in (octa, cube):
        m = 3000
        s = rng.uniform(0.01, 0.2, (m, 1, 1)) * np.where(rng.random((m, 1, 3)) < 0.5, 1.0, rng.uniform(0.9, 1.1, (m, 1, 3)))
        off = np.where(rng.random((m, 1, 1)) < 0.3, 0.0, rng.uniform(-2, 2, (m, 1, 3)))
        put(shape[None] * s + off + rng.normal(0, 1, (m, len(shape), 3)) * rng.choice([0.0, 1e-4, 1e-3], (m, 1, 1)), "isotropic")
    put(rng.uniform(-0.05, 0.05, (4000, 12, 3)) + rng.uniform(-1, 1, (4000, 1, 3)), "blob")
    # regular polygons in an exact plane: a zero eigenvalue and two equal ones (the discriminant of n_roots2 is a rounding decision)
    for sides in (4, 6, 8):
        m = 2000
        ang = 2 * np.pi * np.arange(sides) / sides + rng.uniform(0, 2 * np.pi, (m, 1))
        rad = rng.uniform(0.01, 0.5, (m, 1))
        p = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.zeros((m, sides))], 2) + rng.uniform(-2, 2, (m, 1, 3)) * rng.choice([0.0, 1.0], (m, 1, 1))
        p[:, :, 2] = rng.choice([0.5, 1.0, 2.0, -1.0], (m, 1))
        put(p[:, :, rng.permutation(3)] if sides == 6 else p, "polygon")
    put(_patches(rng, 4000, 6, lo=0.05, hi=0.5), "patch_near")
    put(_patches(rng, 2000, 30), "patch")
    return np.concatenate(acc), np.concatenate(cnt), np.concatenate(first), {t: np.concatenate(v) for t, v in tags.items()}


def _tag_normal(c, idx, acc, cnt, prefix="", count_branch=True):
    """branch names of the rows idx (sums acc, counts cnt) from the restated predicates"""
    P = normal_predicates(acc, cnt)
    ge3 = cnt >= 3
    if count_branch:
        c.split(prefix + "n_plane_normal.count<3", idx, ~ge3)
    for nm, v in P.items():
        if nm.startswith("_"):
            continue
        dom = ge3 & (P[_PRED_DOMAIN[nm]] if nm in _PRED_DOMAIN else True)
        c.split(prefix + nm, idx, v & dom, ~v & dom)


def _case_plane_normal(voxels=None):
    c = Case("n_plane_normal")
    rng = np.random.default_rng(16)
    acc, cnt, first, tags = _branch_sets()
    # known / specials
    base = np.concatenate([sums_f32(_patches(rng, 1, 12))[0], [0.1, -0.2, 1.0]]).astype(F)
    s = _with_specials(base, list(range(12)))
    c.add(words(s[:, :9], np.full(len(s), 12, np.uint32), s[:, 9:]), "known")
    # branch sets, view point = the first point; the exact planes twice more with a view point on either side of the plane
    idx = c.add(words(acc, cnt, first), "branch")
    _tag_normal(c, idx, acc, cnt)
    for t in ("collinear", "coincident", "coincident_generic", "three_points", "nan_in_sums", "isotropic"):
        c.tag("set:" + t, idx[tags[t]])
    nan_rows = np.concatenate([tags["count<3"], tags["coincident"]])
    c.expect["nan_normal"] = (idx[nan_rows], None)
    c.split("n_plane_normal.z>0", idx, np.isin(np.arange(len(idx)), np.concatenate([tags["patch"], tags["three_points"]])), np.isin(np.arange(len(idx)), nan_rows))
    # before the flip an exact plane's normal is +z (v1 = row0 x row1), -y (v2 = row0 x row2), +x (v3 = row1 x row2)
    want = {"plane_z": (2, 1.0), "plane_y": (1, -1.0), "plane_x": (0, 1.0)}
    for t, (axis, sign) in want.items():
        j = tags[t]
        for side, flip in ((3.0, False), (-3.0, True)):
            vp = np.zeros((len(j), 3), F)
            vp[:, axis] = -side * sign           # cos_theta = -vp . n
            k = c.add(words(acc[j], cnt[j], vp), "branch", "n_plane_normal.cos_theta<0/" + ("yes" if flip else "no"))
            e = np.zeros((len(j), 4), F); e[:, axis] = -sign if flip else sign
            c.expect["plane_%s_%s" % (t, "flip" if flip else "keep")] = (k, e)
            c.tag("n_plane_normal.l1 largest/" + ("yes" if t == "plane_z" else "no"), k)
            if t != "plane_z":
                c.tag("n_plane_normal.l2 largest/" + ("yes" if t == "plane_y" else "no"), k)
    # dense
    dacc, dcnt, dfirst = _dense_sums()
    vp = dfirst.copy()
    third = len(vp) // 3
    vp[:third] = dacc[:third, 6:9] / dcnt[:third, None].astype(F)         # the centroid, as the device has it
    vp[third:2 * third] = rng.uniform(-1, 1, (third, 3)).astype(F)
    c.add(words(dacc, dcnt, vp), "dense")
    if voxels is not None:
        vacc, vcnt = neighbourhood_sums(*voxels)
        c.add(words(vacc, vcnt, np.asarray(voxels[0], F).reshape(-1, 3)), "dense")
    # boundary: view points in the plane through the origin (cos_theta ~ 0), counts around 3
    j = np.concatenate([tags["plane_z"], tags["plane_y"], tags["plane_x"]])
    c.add(words(acc[j], cnt[j], np.zeros((len(j), 3), F)), "boundary")
    c.add(words(acc[j], np.full(len(j), 2, np.uint32), first[j]), "boundary")
    return c.finish()


def _case_normal_cen(voxels=None):
    """DP_NORMAL_CEN rows for plane_normal_wave: count >= 3 only (its contract)"""
    c = Case("normal_cen")
    rng = np.random.default_rng(28)
    acc, cnt, first, tags = _branch_sets()
    ok = cnt >= 3
    base = sums_f32(_patches(rng, 1, 12))[0]
    s = _with_specials(base, list(range(9)))
    c.add(words(s, np.full(len(s), 12, np.uint32)), "known")
    idx = c.add(words(acc[ok], cnt[ok]), "branch")
    _tag_normal(c, idx, acc[ok], cnt[ok], count_branch=False)
    dacc, dcnt, _ = _dense_sums()
    c.add(words(dacc, dcnt), "dense")
    if voxels is not None:
        vacc, vcnt = neighbourhood_sums(*voxels)
        c.add(words(vacc[vcnt >= 3], vcnt[vcnt >= 3]), "dense")
    j = np.concatenate([tags["plane_z"], tags["plane_y"], tags["plane_x"]])
    c.add(words(acc[j], np.full(len(j), 3, np.uint32)), "boundary")
    return c.finish()


def _colours(rng, n):
    """n colours: a third random floats, a third integers, a sixth greys, a sixth dark"""
    k = n // 6
    g = rng.integers(0, 256, (k, 1)).astype(np.float64)
    return np.concatenate([rng.uniform(0, 255, (2 * k, 3)), rng.integers(0, 256, (n - 5 * k, 3)).astype(np.float64), np.tile(g, (1, 3)) + rng.choice([0.0, 0.0, 0.37], (k, 1)),
                           rng.uniform(0, 30, (k, 3)), rng.integers(0, 30, (k, 3)).astype(np.float64)])[rng.permutation(n)].astype(F)


def _case_region_from_acc():
    c = Case("a_region_from_acc")
    rng = np.random.default_rng(24)
    acc, cnt, first, tags = _branch_sets()
    rgb = _colours(rng, len(acc))
    base = np.concatenate([sums_f32(_patches(rng, 1, 12))[0], [120.5, 33.25, 7.0]]).astype(F)
    s = _with_specials(base, list(range(12)))
    c.add(words(s, np.full(len(s), 12, np.uint32)), "known")
    idx = c.add(words(acc, rgb, cnt), "branch")
    _tag_normal(c, idx, acc, cnt, "a_region_from_acc:")
    dacc, dcnt, _ = _dense_sums()
    c.add(words(dacc, _colours(rng, len(dacc)), dcnt), "dense")
    return c.finish()


# ---------------------------------------------------------------------------------------------------------------------------------
# distances and colours
# ---------------------------------------------------------------------------------------------------------------------------------
def _centroids(rng, n, transform_share=0.3):
    p = _unit(rng.normal(0, 1, (n, 3))) * rng.uniform(0.3, 12.0, (n, 1))
    t = rng.random(n) < transform_share
    z = np.abs(p[:, 2]) + 0.3
    p[t] = np.stack([p[t, 0] / z[t], p[t, 1] / z[t], np.log(z[t])], 1)
    return p


def _normals(rng, n):
    v = _unit(rng.normal(0, 1, (n, 3)))
    s = np.where(rng.random((n, 1)) < 0.5, 1.0, rng.uniform(0.2, 2.0, (n, 1)))        # unit and non-unit
    return v * s


def _case_voxel_distance():
    c = Case("n_voxel_distance")
    rng = np.random.default_rng(15)
    base = np.array([0.5, -0.3, 2.0, 120, 30, 7, 0.6, 0.0, 0.8, 0.52, -0.28, 2.1, 100, 50, 9, 0.0, 0.6, 0.8, 0.08, 1.0, 0.2, 0.4], F)
    c.add(words(_with_specials(base, list(range(22)))), "known")
    n = DENSE
    ce = _centroids(rng, n)
    seed = rng.choice(np.array([0.08, 0.2, 0.1, 0.05], F), n)
    v = ce + rng.uniform(-1, 1, (n, 3)) * seed[:, None]
    w = np.where(rng.random((n, 1)) < 0.5, np.array([[1.0, 0.2, 0.4]]), rng.uniform(0, 2, (n, 3)))
    c.add(words(ce.astype(F), _colours(rng, n), _normals(rng, n).astype(F), v.astype(F), _colours(rng, n), _normals(rng, n).astype(F), seed, w.astype(F)), "dense")
    # equal rows (every difference an exact zero), parallel and orthogonal unit normals (1 - |dot| at its ends)
    m = 64
    ce = _centroids(rng, m).astype(F); col = _colours(rng, m); nr = _unit(rng.normal(0, 1, (m, 3))).astype(F)
    orth = _unit(np.cross(nr, [0.3, 1.0, 0.2])).astype(F)
    par = np.full((m, 4), [0.08, 1.0, 0.2, 0.4], F)
    c.add(words(ce, col, nr, ce, col, nr, par), "boundary"); c.add(words(ce, col, nr, ce, col, -nr, par), "boundary"); c.add(words(ce, col, nr, ce, col, orth, par), "boundary")
    return c.finish()


def _case_rgb2lab():
    c = Case("n_rgb2lab")
    rng = np.random.default_rng(16)
    c.add(words(np.array([[0, 0, 0], [255, 255, 255], [255, 255, 0], [123, 10, 200], [255, 0, 0], [0, 255, 0], [0, 0, 255]], F)), "known")
    c.add(words(_with_specials([120.0, 30.0, 7.0], [0, 1, 2])), "known")
    g = np.linspace(0, 255, 17)
    c.add(words(np.array([[r, gg, b] for r in g for gg in g for b in g], F)), "known")           # the lattice of tests/test_pins.py
    # branches: each channel below / above the gamma knee (v = 0.01 against 0.5), X, Y, Z below / above the knee of f
    cand = np.concatenate([_colours(rng, 600), rng.uniform(0, 40, (600, 3)).astype(F), np.where(rng.random((600, 3)) < 0.5, F(2.55), F(127.5)).astype(F)])
    idx = c.add(words(cand), "branch")
    _, (v, X, Y, Z) = lab_f64(cand)
    for ch in range(3):
        c.split("n_rgb2lab.v<=0.04045 channel %d" % ch, idx, v[:, ch] <= 0.04045 * 0.9, v[:, ch] > 0.04045 * 1.1)
    for nm, t in (("n_lab_f(X).t>0.008856", X), ("n_rgb2lab.Y>0.008856", Y), ("n_lab_f(Z).t>0.008856", Z)):
        c.split(nm, idx, t > 0.008856 * 1.1, t <= 0.008856 * 0.9)
    n = DENSE
    c.add(words(rng.uniform(0, 255, (n, 3)).astype(F)), "dense")
    c.add(words(rng.integers(0, 256, (n, 3)).astype(F)), "dense")
    c.add(words(_colours(rng, 60000)), "dense")
    # boundaries: a channel at the gamma knee; greys and single channels where X, Y or Z crosses 0.008856 (bisection in float64)
    knee = _ulps32(np.array([0.04045 * 255.0], F), np.arange(-6, 7))
    rows = [np.stack([knee, np.full_like(knee, 90), np.full_like(knee, 200)], 1), np.stack([np.full_like(knee, 3), knee, knee], 1), np.stack([knee, knee, knee], 1)]
    for which in range(3):
        for shape in ([1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0.5]):
            lo, hi = 0.0, 255.0
            for _ in range(60):
                mid = (lo + hi) / 2
                val = lab_f64(np.array([shape], np.float64) * mid)[1][1 + which][0]
                lo, hi = (mid, hi) if val < 0.008856 else (lo, mid)
            if hi < 254:
                t = _ulps32(np.array([hi], F), np.arange(-6, 7))
                rows.append(np.outer(t, np.array(shape, F)).astype(F))
    c.add(words(np.concatenate(rows).astype(F)), "boundary")
    return c.finish()


def _lch(L, C, hdeg):
    h = np.radians(hdeg)
    return np.stack([L, C * np.cos(h), C * np.sin(h)], 1).astype(F)


def _case_ciede00(lab_of, name="n_ciede00"):
    c = Case(name)
    rng = np.random.default_rng(17)
    k = np.array(KAT["ciede2000"], np.float64)
    idx = c.add(words(np.concatenate([k[:, 0:6], np.hstack([k[:, 3:6], k[:, 0:3]])]).astype(F)), "known")
    c.expect["kat"] = (idx, np.concatenate([k[:, 6], k[:, 6]]))
    c.add(words(_with_specials([50.0, 2.5, -30.0, 61.0, -5.0, 29.0], list(range(6)))), "known")
    # branches.  candidates in L C h form; the float64 restatement decides with a margin of 3 degrees
    m = 4000
    h1 = rng.choice([10.0, 80.0, 170.0, 200.0, 275.0, 350.0], m) + rng.uniform(-4, 4, m)
    h2 = rng.choice([10.0, 100.0, 185.0, 200.0, 355.0, 350.0], m) + rng.uniform(-4, 4, m)
    l1 = _lch(rng.uniform(5, 95, m), rng.uniform(5, 60, m), h1); l2 = _lch(rng.uniform(5, 95, m), rng.uniform(5, 60, m), h2)
    idx = c.add(words(l1, l2), "branch")
    _, p = ciede2000_f64(l1, l2)
    mg = 3.0
    c.split("n_ciede00.hp1<0", idx, (p["h1"] > 180 + mg) & (p["h1"] < 360 - mg), (p["h1"] > mg) & (p["h1"] < 180 - mg))
    c.split("n_ciede00.hp2<0", idx, (p["h2"] > 180 + mg) & (p["h2"] < 360 - mg), (p["h2"] > mg) & (p["h2"] < 180 - mg))
    c.split("n_ciede00.dhp>PI", idx, p["dh"] > 180 + mg, p["dh"] < 180 - mg)
    c.split("n_ciede00.dhp<-PI", idx, p["dh"] < -180 - mg, (p["dh"] > -180 + mg) & (p["dh"] <= 180 - mg))
    wide = np.abs(p["dh"]) > 180 + mg
    c.split("n_ciede00.|hp1-hp2|>PI", idx, wide, np.abs(p["dh"]) < 180 - mg)
    c.split("n_ciede00.hp<0 after -PI", idx, wide & (p["hs"] < 360 - 2 * mg), wide & (p["hs"] > 360 + 2 * mg))
    # greys: exact zeros in a and b on one side or on both
    m = 48
    col = _lch(rng.uniform(5, 95, m), rng.uniform(5, 60, m), rng.uniform(0, 360, m))
    grey = np.stack([rng.uniform(0, 100, m), np.zeros(m), np.zeros(m)], 1).astype(F)
    grey[::4, 1] = -0.0; grey[1::4, 2] = -0.0
    for a, b, t1, t2 in ((grey, col, "yes", "no"), (col, grey, "no", "yes"), (grey, grey[::-1], "yes", "yes")):
        idx = c.add(words(a, b), "branch", ["n_ciede00.chroma1==0/" + t1, "n_ciede00.chroma2==0/" + t2, "n_ciede00.Cp_prod==0/yes"])
        c.expect.setdefault("grey", []).append(idx)
    idx = c.add(words(col, col[::-1]), "branch", ["n_ciede00.chroma1==0/no", "n_ciede00.chroma2==0/no", "n_ciede00.Cp_prod==0/no"])
    c.expect["grey"] = (np.concatenate(c.expect["grey"]), None)
    # dense: Lab of random and of all-integer 8-bit colours through n_rgb2lab (lab_of), pairs of unrelated and of similar colours
    n = DENSE
    a = _colours(rng, n)
    b = _colours(rng, n)
    sim = rng.random(n) < 0.4
    b[sim] = np.clip(a[sim] + rng.normal(0, 10, (int(sim.sum()), 3)), 0, 255).astype(F)
    integer = rng.random(n) < 0.5
    b[integer] = np.round(b[integer]); a[integer] = np.round(a[integer])
    c.add(words(lab_of(a), lab_of(b)), "dense")
    # boundary: opposite hues (dhp = +-PI up to rounding), hues at 0 / 2 PI, chroma near zero, equal colours
    m = 400
    h = rng.uniform(0, 360, m); C1 = rng.uniform(1, 60, m); C2 = rng.uniform(1, 60, m)
    l1 = _lch(rng.uniform(5, 95, m), C1, h)
    rows = [np.hstack([l1, np.stack([rng.uniform(5, 95, m).astype(F), -l1[:, 1] * F(0.5), -l1[:, 2] * F(0.5)], 1)])]
    l2 = l1.copy(); l2[:, 0] = rng.uniform(5, 95, m); l2[:, 1:] *= -1
    rows.append(np.hstack([l1, l2])); rows.append(np.hstack([l2, l1])); rows.append(np.hstack([l1, l1]))
    tiny = np.concatenate([FS[2:8], _ulps32(np.array([1e-30, 1e-20, 1e-10], F), [0, 1])]).astype(F)
    t = np.array([[50, x, y, 60, 20, -10] for x in tiny for y in tiny], F)
    rows.append(t); rows.append(t[:, [3, 4, 5, 0, 1, 2]])
    ax = _ulps32(np.array([1e-6, 1e-3], F), [0])
    t = np.array([[50, 20, s * e, 60, 25, s2 * e] for e in np.concatenate([ax, tiny[:4]]) for s in (1, -1) for s2 in (1, -1)], F)          # hues just either side of 0 / 2 PI
    rows.append(t)
    g = rng.integers(0, 256, (600, 1)).astype(F)
    rows.append(np.hstack([lab_of(np.tile(g, (1, 3))), lab_of(np.tile(g[::-1], (1, 3)))]))          # greys through n_rgb2lab: chroma of rounding size
    c.add(words(np.concatenate(rows).astype(F)), "boundary")
    return c.finish()


def _case_rgb_eucl():
    c = Case("n_rgb_eucl")
    rng = np.random.default_rng(18)
    a = np.array([r[0] for r in KAT["rgb_eucl"]] + [[0, 0, 0]], F); b = np.array([r[1] for r in KAT["rgb_eucl"]] + [[255, 255, 255]], F)
    want = np.array([r[2] for r in KAT["rgb_eucl"]] + [KAT["RGB_RANGE"]], np.float64)
    idx = c.add(words(np.concatenate([a, b]), np.concatenate([b, a])), "known")
    c.expect["kat"] = (idx, np.concatenate([want, want]))
    c.add(words(_with_specials([120.0, 30.0, 7.0, 119.0, 200.0, 7.5], list(range(6)))), "known")
    c.add(words(_colours(rng, DENSE), _colours(rng, DENSE)), "dense")
    x = _colours(rng, 500)
    c.add(words(x, x), "boundary")
    c.add(words(x, np.nextafter(x, F(300))), "boundary")
    return c.finish()


def _geom_rows(rng, n):
    c1 = _centroids(rng, n)
    c2 = c1 + rng.uniform(-0.3, 0.3, (n, 3))
    return _normals(rng, n).astype(F), c1.astype(F), _normals(rng, n).astype(F), c2.astype(F)


def _convex_margin(n1, c1, n2, c2):
    n1, c1, n2, c2 = (np.asarray(v, F).astype(np.float64) for v in (n1, c1, n2, c2))
    C = _unit(c1 - c2)
    return (n1 * C).sum(1) - (n2 * C).sum(1)


def _case_geom(name):
    c = Case(name)
    rng = np.random.default_rng(FN[name])
    base = np.array([0.6, 0.0, 0.8, 0.5, -0.3, 2.0, 0.0, 0.6, 0.8, 0.58, -0.25, 2.1], F)
    c.add(words(_with_specials(base, list(range(12)))), "known")
    g = _geom_rows(rng, 200)
    idx = c.add(words(*g), "branch")
    mg = _convex_margin(*g)
    c.split("n_is_convex.cos1>=cos2", idx, mg > 0.05, mg < -0.05)
    c.add(words(*_geom_rows(rng, DENSE)), "dense")
    n1, c1, n2, c2 = _geom_rows(rng, 300)
    c.add(words(n1, c1, n1, c2), "boundary")                # equal normals: cos1 == cos2
    c.add(words(n1, c1, n2, c1), "boundary")                # equal centroids: 0 / 0
    c.add(words(n1, c1, -n1, c2), "boundary")
    perp = _unit(np.cross(c1 - c2, [0.2, 1.0, 0.3])).astype(F)
    c.add(words(perp, c1, n2, c2), "boundary")              # n1 orthogonal to the line of centres
    return c.finish()


def _records(rng, n, lab_of):
    """region records without the spare words: centroid, normal, mean rgb, Lab of the mean (12 floats), pairs of neighbours"""
    n1, c1, n2, c2 = _geom_rows(rng, n)
    a = _colours(rng, n); b = _colours(rng, n)
    sim = rng.random(n) < 0.5
    b[sim] = np.clip(a[sim] + rng.normal(0, 10, (int(sim.sum()), 3)), 0, 255).astype(F)
    return np.hstack([c1, n1, a, lab_of(a)]).astype(F), np.hstack([c2, n2, b, lab_of(b)]).astype(F)


def _case_delta_c_g(lab_of):
    c = Case("n_delta_c_g")
    rng = np.random.default_rng(21)
    r1, r2 = _records(rng, 1, lab_of)
    s = _with_specials(np.concatenate([r1[0], r2[0]]), list(range(24)))
    for cm in (0, 1):
        for gm in (0, 1):
            c.add(words(s, np.full(len(s), cm, np.uint32), np.full(len(s), gm, np.uint32)), "known")
    r1, r2 = _records(rng, 400, lab_of)
    cm = rng.integers(0, 2, 400).astype(np.uint32); gm = rng.integers(0, 2, 400).astype(np.uint32)
    idx = c.add(words(r1, r2, cm, gm), "branch")
    mg = _convex_margin(r1[:, 3:6], r1[:, 0:3], r2[:, 3:6], r2[:, 0:3])
    c.split("n_delta_c_g.color_metric==0", idx, cm == 0)
    c.split("n_delta_c_g.geom_metric==1", idx, gm == 1)
    c.split("n_delta_c_g.convex halves", idx, (gm == 1) & (mg > 0.05), (gm == 1) & (mg < -0.05))
    n = DENSE
    r1, r2 = _records(rng, n, lab_of)
    c.add(words(r1, r2, rng.integers(0, 2, n).astype(np.uint32), rng.integers(0, 2, n).astype(np.uint32)), "dense")
    r1, r2 = _records(rng, 300, lab_of)
    r2[:, 3:6] = r1[:, 3:6]
    c.add(words(r1, r2, np.zeros(300, np.uint32), np.ones(300, np.uint32)), "boundary")          # equal normals: the convexity test ties
    return c.finish()


def _case_weight_key():
    c = Case("n_weight_key")
    rng = np.random.default_rng(22)
    c.add(words(np.concatenate([FS, np.array([1.0, -1.0, 0.5, 2.0], F)])), "known")
    c.add(rng.integers(0, 2 ** 32, (20000, 1), dtype=np.uint64).astype(np.uint32), "known")
    nan = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffffffff, 0x7fa00000, 0xffa12345], np.uint32)
    num = rng.uniform(-2, 2, 16).astype(F)
    c.split("n_weight_key.nan", c.add(np.concatenate([nan, num.view(np.uint32)])[:, None], "branch"), np.arange(24) < 8)
    z = np.concatenate([np.full(8, 0x80000000, np.uint32), np.zeros(4, np.uint32), rng.uniform(-1, 1, 8).astype(F).view(np.uint32)])
    c.split("n_weight_key.minus_zero", c.add(z[:, None], "branch"), z == 0x80000000)
    s = rng.uniform(0.01, 2, 32).astype(F) * np.repeat([F(-1), F(1)], 16)
    c.split("n_weight_key.sign", c.add(s.view(np.uint32)[:, None], "branch"), s < 0)
    c.add(rng.uniform(0, 2, DENSE).astype(F).view(np.uint32)[:, None], "dense")
    c.add(rng.integers(0, 2 ** 32, (DENSE, 1), dtype=np.uint64).astype(np.uint32), "dense")
    e = np.array([0, 0x80000000, 0x7f800000, 0xff800000], np.int64)
    c.add(((e[:, None] + np.arange(-4, 5)[None, :]) & 0xFFFFFFFF).astype(np.uint32).reshape(-1, 1), "boundary")
    return c.finish()


def _case_fold():
    c = Case("a_fold")
    rng = np.random.default_rng(23)

    def rows(n, k):
        xyz = (_centroids(rng, n)[:, None, :] + rng.uniform(-0.05, 0.05, (n, FOLD_MAX, 3))).astype(F)
        rgb = np.where(rng.random((n, FOLD_MAX, 1)) < 0.5, rng.integers(0, 256, (n, FOLD_MAX, 3)).astype(np.float64), rng.uniform(0, 255.99, (n, FOLD_MAX, 3))).astype(F)
        feat = np.concatenate([xyz, rgb], 2)
        k = np.broadcast_to(np.asarray(k, np.uint32), (n,))
        feat[np.arange(FOLD_MAX)[None, :] >= k[:, None]] = 0
        return words(k, feat.reshape(n, -1))

    s = _with_specials(np.concatenate([[0.5, -0.3, 2.0, 120, 30, 7]] * FOLD_MAX), [0, 1, 2, 6, 7, 8, 42, 43, 44])
    c.add(words(np.full(len(s), FOLD_MAX, np.uint32), s), "known")
    for k in range(FOLD_MAX + 1):
        idx = c.add(rows(16, k), "branch", "set:a_fold.rows==%d" % k)
        c.tag("a_fold.rows==3/" + ("yes" if k == 3 else "no"), idx)
    c.add(rows(DENSE, rng.integers(1, FOLD_MAX + 1, DENSE)), "dense")
    return c.finish()


def _cdf(rng, n):
    return np.sort(rng.random((n, CDF)), 1).astype(F)


def _case_t(name):
    """a_tc / a_tg rows: merging lambda bins d cdf[8]"""
    c = Case(name)
    tc = name == "a_tc"
    rng = np.random.default_rng(FN[name])
    bc = lambda v, t, n: np.broadcast_to(np.asarray(v, t), (n,))
    row = lambda merging, lam, bins, d, cdf: words(bc(merging, np.uint32, len(cdf)), bc(lam, F, len(cdf)), bc(bins, np.uint32, len(cdf)), bc(d, F, len(cdf)), cdf)
    for merging in (0, 1):                                   # lambda * d: every special in both
        s = _with_specials([0.5, 0.3], [0, 1])
        c.add(row(np.full(len(s), merging), s[:, 0], np.full(len(s), 5), s[:, 1], _cdf(rng, len(s))), "known")
    m = 48
    merging = np.repeat([0, 1, 2], 16)
    idx = c.add(row(merging, rng.random(m), rng.integers(1, CDF + 1, m), rng.uniform(0, 0.99, m), _cdf(rng, m)), "branch")
    c.split(name + ".merging!=2", idx, merging != 2)
    bins = np.tile(np.arange(1, CDF + 1), 2)
    two = np.full(len(bins), 2)
    idx = c.add(row(two, 0.5, bins, np.ones(len(bins)), _cdf(rng, len(bins))), "branch", (name + ".bin==bins/yes") if tc else (name + ".err/yes"))     # d = 1: a_tc steps back, a_tg refuses
    c.expect["top"] = (idx, bins)
    idx = c.add(row(two, 0.5, bins, rng.uniform(0.01, 0.99, len(bins)), _cdf(rng, len(bins))), "branch", [name + ".err/no", name + ".d*bins integral/no"] + ([name + ".bin==bins/no"] if tc else []))
    idx = c.add(row(two, 0.5, bins, -rng.uniform(0.01, 3.0, len(bins)), _cdf(rng, len(bins))), "branch", [name + ".err/yes", name + ".bin<0/yes"])
    c.expect["err_low"] = (idx, None)
    idx = c.add(row(two, 0.5, bins, rng.uniform(2.1, 40.0, len(bins)), _cdf(rng, len(bins))), "branch", [name + ".err/yes", name + ".bin>=bins/yes", name + ".bin<0/no"])
    c.expect["err_high"] = (idx, None)               # (d >= 2: past the one bin that a_tc's bin == bins step forgives)
    # d * bins integral: d = k / bins, exact for bins 1, 2, 4, 8 and rounded for the others
    kb = np.array([[k, b] for b in range(1, CDF + 1) for k in range(0, b)])
    d = (kb[:, 0] / kb[:, 1]).astype(F)
    idx = c.add(row(np.full(len(kb), 2), 0.5, kb[:, 1], d, _cdf(rng, len(kb))), "branch", [name + ".d*bins integral/yes", name + ".bin>=bins/no"])
    pw = np.isin(kb[:, 1], [1, 2, 4, 8])
    c.expect["integral"] = (idx[pw], kb[pw, 0])
    n = DENSE
    c.add(row(rng.choice([0, 1, 2, 2], n), rng.random(n), rng.integers(1, CDF + 1, n), rng.random(n), _cdf(rng, n)), "dense")
    dd = _ulps32(d[d > 0], KS); bb = np.repeat(kb[d > 0, 1], len(KS))
    c.add(row(np.full(len(dd), 2), 0.5, bb, dd, _cdf(rng, len(dd))), "boundary")
    return c.finish()


def _case_edge_weight(name, lab_of):
    """a_edge_weight rows; name a_edge_weight_lab: colour metric LAB_CIEDE00 only (what edge_weight_quad restates)"""
    c = Case(name)
    lab_only = name.endswith("_lab")
    rng = np.random.default_rng(27 + lab_only)

    def rows(n, merging, r=None, cm=None):
        r1, r2 = _records(rng, n, lab_of) if r is None else r
        cm = (np.zeros(n) if lab_only else rng.integers(0, 2, n)) if cm is None else cm
        gm = rng.integers(0, 2, n)
        return words(r1, r2, np.asarray(cm, np.uint32), gm.astype(np.uint32), np.asarray(merging, np.uint32), rng.random(n).astype(F), rng.integers(1, CDF + 1, n).astype(np.uint32),
                     _cdf(rng, n), _cdf(rng, n)), cm, gm

    r1, r2 = _records(rng, 1, lab_of)
    s = _with_specials(np.concatenate([r1[0], r2[0]]), list(range(24)))
    for merging in (0, 1):                                   # (EQUALIZATION takes no NaN: see the module docstring)
        c.add(rows(len(s), np.full(len(s), merging), (s[:, :12], s[:, 12:]))[0], "known")
    for merging in (0, 1, 2):
        w, cm, gm = rows(64, np.full(64, merging))
        idx = c.add(w, "branch", "a_edge_weight.merging==%d/yes" % merging)
        for other in (0, 1, 2):
            if other != merging:
                c.tag("a_edge_weight.merging==%d/no" % other, idx)
        if not lab_only:
            c.split("a_edge_weight.color_metric==0 (merging %d)" % merging, idx, cm == 0)
        c.split("a_edge_weight.geom_metric==1 (merging %d)" % merging, idx, gm == 1)
    n = DENSE
    c.add(rows(n, rng.choice([0, 1, 2, 2], n))[0], "dense")
    r1, r2 = _records(rng, 300, lab_of)
    c.add(rows(300, np.full(300, 1), (r1, r1))[0], "boundary")                 # a region against itself: dc = 0, centroids equal (dg = 0 / 0: only under the lambda modes)
    r2[:, 3:6] = r1[:, 3:6]
    c.add(rows(300, np.full(300, 2), (r1, r2))[0], "boundary")
    return c.finish()


_cache = {}


def case(name, lab_of=None, voxels=None):
    """The rows of one function.  lab_of: float32 rgb (n, 3) -> float32 Lab (n, 3), n_rgb2lab of the host probe when the caller has it
    (a float64 formula otherwise); voxels: (VOXEL_XYZ, VOXEL_NEIGHBORS) of the oracle on the fixture frame, for the dense rows of real
    voxel neighbourhoods.  Results are cached per name."""
    if name in _cache:
        return _cache[name]
    lab_of = lab_of or _lab_default
    if FN[name] <= 10:
        c = _case_math(name)
    else:
        c = {"n_transform": _case_transform, "n_point_key": _case_point_key, "n_morton": _case_morton,
             "n_plane_normal": lambda: _case_plane_normal(voxels), "normal_cen": lambda: _case_normal_cen(voxels),
             "a_region_from_acc": _case_region_from_acc, "n_voxel_distance": _case_voxel_distance, "n_rgb2lab": _case_rgb2lab,
             "n_ciede00": lambda: _case_ciede00(lab_of), "n_ciede00_sq": lambda: _case_ciede00(lab_of, "n_ciede00_sq"), "n_rgb_eucl": _case_rgb_eucl, "n_normals_diff": lambda: _case_geom("n_normals_diff"),
             "n_is_convex": lambda: _case_geom("n_is_convex"), "n_delta_c_g": lambda: _case_delta_c_g(lab_of), "n_weight_key": _case_weight_key,
             "a_fold": _case_fold, "a_tc": lambda: _case_t("a_tc"), "a_tg": lambda: _case_t("a_tg"),
             "a_edge_weight": lambda: _case_edge_weight("a_edge_weight", lab_of), "a_edge_weight_lab": lambda: _case_edge_weight("a_edge_weight_lab", lab_of)}[name]()
    _cache[name] = c
    return c


NAMES = list(FN)


# ---------------------------------------------------------------------------------------------------------------------------------
# sparse contingency tables for evl_scores (the arrays of dp_host_evl / dp_dev_evl)
# ---------------------------------------------------------------------------------------------------------------------------------
def pack_tables(tables):
    """tables: list of (dense K x M table, ssize, tsize, N) -> dict of the concatenated CSR arrays and the dims rows of devprobe_fns.h"""
    dims, ss, ts, ro, co, cn = [], [], [], [], [], []
    ok = om = oe = 0
    for t, (table, ssize, tsize, N) in enumerate(tables):
        table = np.asarray(table, np.uint32)
        K, M = table.shape
        assert K >= 1 and M >= 1 and len(ssize) == K and len(tsize) == M
        i, j = np.nonzero(table)              # row-major: rows ascending, columns ascending inside a row
        roff = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=K))]).astype(np.uint32)
        dims.append([K, M, int(N), ok, om, ok + t, oe, 0])
        ss.append(np.asarray(ssize, np.uint32)); ts.append(np.asarray(tsize, np.uint32)); ro.append(roff)
        co.append(j.astype(np.uint32)); cn.append(table[i, j].astype(np.uint32))
        ok += K; om += M; oe += len(i)
    cat = lambda l: np.ascontiguousarray(np.concatenate(l).astype(np.uint32))
    return dict(T=len(tables), dims=np.array(dims, np.uint32), ssize=cat(ss), tsize=cat(ts), roff=cat(ro), col=cat(co), cnt=cat(cn), nk=ok, nm=om, ne=oe)


# ---------------------------------------------------------------------------------------------------------------------------------
# output rows: what each word is (f float32, u integer, d one half of a float64: always in pairs), for NaN-aware comparison
# ---------------------------------------------------------------------------------------------------------------------------------
OUT_KIND = {fn: "dd" for fn in range(11)}
OUT_KIND.update({11: "fff", 12: "uuuuuu" + "d" * 12, 13: "u" * 7, 14: "ffff", 15: "f", 16: "fff", 17: "f", 18: "f", 19: "f", 20: "u", 21: "ff", 22: "u",
                 23: "f" * 12, 24: "f" * 16, 25: "fu", 26: "fu", 27: "fu", 28: "f" * 7, 29: "dd"})


def typed(out, kind):
    """the float32, float64 and integer words of output rows as three arrays (n, columns of that type)"""
    out = np.ascontiguousarray(out, np.uint32)
    assert out.shape[1] == len(kind), (out.shape, kind)
    col = lambda ch: [i for i, k in enumerate(kind) if k == ch]
    d = np.ascontiguousarray(out[:, col("d")])
    return np.ascontiguousarray(out[:, col("f")]).view(F), d.view(np.float64) if d.shape[1] else d.view(F), np.ascontiguousarray(out[:, col("u")])


def rows_equal(got, want, kind):
    """per row: every word equal, except that a NaN matches a NaN (conftest.same_bits, row by row)"""
    ok = np.ones(len(got), bool)
    for a, b in zip(typed(got, kind), typed(want, kind)):
        if a.shape[1] == 0:
            continue
        if a.dtype.kind == "f":
            w = a.view(np.uint32 if a.dtype == F else np.uint64) == b.view(np.uint32 if a.dtype == F else np.uint64)
            ok &= (w | (np.isnan(a) & np.isnan(b))).all(1)
        else:
            ok &= (a == b).all(1)
    return ok
