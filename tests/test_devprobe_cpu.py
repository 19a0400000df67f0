"""The device probe without a GPU (tests/devprobe/, tests/devprobe_inputs.py): the g++ build of the dispatch table over the per-element
functions of csrc/f3ds_math.h, f3ds_numerics.h, f3ds_algo.h and f3ds_eval_levels.h is the reference side of tests/test_devprobe_gpu.py.
Checked here: the branch bookkeeping of the inputs, that the g++ probe is the arithmetic the suite already trusts (the oracle's and the
emulation's exports, bit for bit), its distance to plain float64 formulas, its flags, and that the device library cross-compiles."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import devprobe_inputs as D
from conftest import FIXTURE_PCD, ROOT, _make, same_bits
from test_eval_levels_cpu import _matching, _random_case, _run as _harness_run, harness  # noqa: F401  (harness: the fixture)

F = np.float32
PROBE_DIR = os.path.join(ROOT, "tests", "devprobe")
ERR9 = np.uint32(0xFFFFFFF7)          # -9 (the reference's map::at would throw)
VP = ctypes.c_void_p


class Probe:
    """ctypes wrapper of one probe library (prefix dp_host or dp_dev): run(fn, rows) -> output rows; a non-zero return code fails."""

    def __init__(self, path, prefix):
        self.lib = ctypes.CDLL(path)
        self.prefix = prefix
        for nm in ("run", "shape", "evl"):
            getattr(self.lib, prefix + "_" + nm).restype = ctypes.c_int

    def shape(self, fn):
        ni, no = ctypes.c_int(), ctypes.c_int()
        assert getattr(self.lib, self.prefix + "_shape")(ctypes.c_int(fn), ctypes.byref(ni), ctypes.byref(no)) == 0, fn
        return ni.value, no.value

    def call(self, entry, rows, no, *head):
        rows = np.ascontiguousarray(rows, np.uint32)
        out = np.zeros((len(rows), no), np.uint32)
        f = getattr(self.lib, self.prefix + "_" + entry)
        f.restype = ctypes.c_int
        rc = f(*head, VP(rows.ctypes.data), VP(out.ctypes.data), ctypes.c_size_t(len(rows)))
        assert rc == 0, "%s_%s returned %d" % (self.prefix, entry, rc)
        return out

    def run(self, fn, rows):
        ni, no = self.shape(fn)
        assert rows.shape[1] == ni, (fn, rows.shape, ni)
        return self.call("run", rows, no, ctypes.c_int(fn))

    def evl(self, pk):
        out = np.zeros((pk["T"], 7), np.uint32)
        args = [ctypes.c_uint32(pk["T"])] + [VP(pk[k].ctypes.data) for k in ("dims", "ssize", "tsize", "roff", "col", "cnt")] + [ctypes.c_size_t(pk["nk"]), ctypes.c_size_t(pk["nm"])]
        if self.prefix == "dp_dev":
            args.append(ctypes.c_size_t(pk["ne"]))
        rc = getattr(self.lib, self.prefix + "_evl")(*args, VP(out.ctypes.data))
        assert rc == 0, "%s_evl returned %d" % (self.prefix, rc)
        return out.view(F)


@pytest.fixture(scope="session")
def hostprobe():
    _make("tests/devprobe")          # (a no-op when both libraries are newer than their sources)
    return Probe(os.path.join(PROBE_DIR, "libf3ds_devprobe_host.so"), "dp_host")


@pytest.fixture(scope="session")
def cases(hostprobe, oracle, P):
    """name -> Case, with Lab through the probe's n_rgb2lab and the one-ring sums of the fixture frame's voxels among the dense rows"""
    rc, _, _, h = oracle.segment(P.read_pcd(FIXTURE_PCD), P.launch_params())
    assert rc == 0
    voxels = (h.get("VOXEL_XYZ").reshape(-1, 3).copy(), h.get("VOXEL_NEIGHBORS").reshape(-1, 27).copy())
    h.close()
    lab_of = lambda rgb: hostprobe.run(D.FN["n_rgb2lab"], D.words(np.asarray(rgb, F))).view(F)
    return lambda name: D.case(name, lab_of, voxels)


def evl_tables(many=True):
    """The tables of tests/test_eval_levels_cpu.py, regenerated with its seeds: [(what, table, ssize, tsize, N)]"""
    out = []
    rng = np.random.default_rng(20261016)
    for it in range(400):
        K = int(rng.integers(1, 40)); M = int(rng.integers(1, 40))
        out.append(("random %d" % it,) + _random_case(rng, K, M, float(rng.uniform(0.05, 0.6)), int(rng.choice([0, 5, 100000]))))
    if many:
        rng = np.random.default_rng(11)
        table, ssize, tsize, N = _random_case(rng, 60, 3000, 0.01, 1000)
        tsize[rng.choice(3000, 1500, replace=False)] = tsize[0]
        tsize = np.maximum(tsize, table.sum(0)).astype(np.uint32)
        out.append(("K 60, M 3000", table, ssize, tsize, int(tsize.sum()) + 1000))
    rng = np.random.default_rng(7)
    for it in range(50):
        M = int(rng.integers(1, 12))
        out.append(("K = 1, case %d" % it,) + _random_case(rng, 1, M, 0.5, int(rng.integers(0, 50))))
        K = int(rng.integers(1, 12))
        out.append(("M = 1, case %d" % it,) + _random_case(rng, K, 1, 0.5, int(rng.integers(0, 50))))
    a = lambda t: np.array(t, np.uint32)
    out += [("1 x 1", a([[3]]), [3], [3], 3), ("1 x 1 empty", a([[0]]), [2], [5], 5),
            ("equal sizes + empty column", a([[0, 2, 0], [3, 4, 0], [3, 0, 0]]), [3, 7, 3], [6, 6, 2], 20),
            ("equal counts + row 0 used", a([[5, 0], [5, 0], [1, 0]]), [5, 6, 1], [11, 1], 12),
            ("column of used rows", a([[4, 1], [0, 0]]), [5, 2], [4, 3], 9), ("large N", a([[4, 1], [0, 0]]), [5, 2], [4, 3], 10 ** 7)]
    return out


# ---- the inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.NAMES)
def test_branch_bookkeeping(cases, name):
    """Every named branch has at least 8 rows on each side; at least 200 000 dense rows per function."""
    c = cases(name)
    assert len(c.groups["dense"]) >= D.DENSE and len(c.groups["known"]) > 0
    names = {b.rsplit("/", 1)[0] for b in c.branches if not b.startswith("set:")}
    for b in sorted(names):
        for side in ("yes", "no"):
            assert len(c.branches.get(b + "/" + side, ())) >= 8, "%s: branch %s/%s has %d rows" % (name, b, side, len(c.branches.get(b + "/" + side, ())))
    assert sum(len(v) for v in c.groups.values()) == len(c.rows)


def test_evl_tables_cover_the_matching_quirks():
    """equal truth sizes, empty columns with row 0 free / used, equal counts, unmatched labels: at least 8 tables on each side"""
    seen = {}
    for what, table, ssize, tsize, N in evl_tables(many=False):
        match, notes = _matching(np.asarray(table), tsize)
        notes = set(notes) | ({"unmatched label"} if -1 in match else set())
        for q in ("equal sizes", "empty column, row 0 free", "empty column, row 0 used", "equal counts", "unmatched label"):
            seen.setdefault((q, q in notes), []).append(what)
    for k, v in seen.items():
        assert len(v) >= 8, (k, len(v))
    assert len(seen) == 10


def test_rows_go_the_way_they_were_built(cases, hostprobe):
    """Wherever the outcome shows the branch, the host probe takes the side the float64 restatement chose."""
    c = cases("n_ciede00"); out = hostprobe.run(c.fn, c.rows).view(F)[:, 0]
    idx, _ = c.expect["grey"]
    f = c.rows[idx].view(F)
    _, p = D.ciede2000_f64(f[:, :3], f[:, 3:])
    assert p["grey"].all()
    want = np.sqrt(p["tL"] ** 2 + p["tC"] ** 2)          # grey: dH == 0
    # half an ulp of the float result (values < 128: 3.8e-6) + the float32 chroma behind G (60 * 1e-7), twice
    assert np.abs(out[idx].astype(np.float64) - want).max() <= 2e-5
    sq = hostprobe.run(D.FN["n_ciede00_sq"], c.rows).view(np.float64)[:, 0]          # the radicand in double: n_ciede00 is its root, rounded once
    with np.errstate(all="ignore"):
        assert same_bits(np.sqrt(sq).astype(F), out)
    for nm in ("n_ciede00", "n_rgb_eucl"):                # the reference's known answers, both argument orders, the existing tolerance
        c = cases(nm); out = hostprobe.run(c.fn, c.rows).view(F)[:, 0]
        idx, want = c.expect["kat"]
        assert np.abs(out[idx] - want).max() < 1e-4, nm

    c = cases("n_plane_normal"); out = hostprobe.run(c.fn, c.rows).view(F)
    assert np.isnan(out[c.expect["nan_normal"][0], :3]).all()          # count < 3, zero covariance
    assert not np.isnan(out[c.branches["n_plane_normal.z>0/yes"], :3]).any()
    for k, (idx, want) in c.expect.items():
        if k.startswith("plane_"):
            assert np.array_equal(out[idx], want), k                    # the eigenvector picked (v1 / v2 / v3) and the flip

    c = cases("n_point_key"); out = hostprobe.run(c.fn, c.rows)
    for k in ("border_on", "border_below", "border_above", "mid_cell", "key_zero"):
        idx, want = c.expect[k]
        assert np.array_equal(out[idx, :3], want), k                    # on a border: key k, not k - 1
    assert (out[c.branches["n_key_bit_size.depth_error/yes"], 5] == np.uint32(-4 & 0xFFFFFFFF)).all() and (out[c.branches["n_key_bit_size.depth_error/no"], 5] == 0).all()
    assert (out[c.branches["n_key_bit_size.k>2/no"], 3] == 1).all()

    c = cases("n_morton"); out = hostprobe.run(c.fn, c.rows)
    x, y, z, d = (c.rows[:, k] for k in range(4))
    code = out[:, 0].astype(np.uint64) | (out[:, 1].astype(np.uint64) << np.uint64(32))
    assert np.array_equal(code, D.morton_py(x, y, z, d))
    mask = ((np.uint64(1) << d.astype(np.uint64)) - np.uint64(1)).astype(np.uint32)
    assert np.array_equal(out[:, 2:5], c.rows[:, :3] & mask[:, None])
    pack = out[:, 5].astype(np.uint64) | (out[:, 6].astype(np.uint64) << np.uint64(32))
    assert np.array_equal(pack, (x.astype(np.uint64) << np.uint64(42)) | (y.astype(np.uint64) << np.uint64(21)) | z.astype(np.uint64))

    c = cases("n_weight_key"); out = hostprobe.run(c.fn, c.rows)[:, 0]
    assert (out[c.branches["n_weight_key.nan/yes"]] == 0xFFFFFFFE).all() and (out[c.branches["n_weight_key.minus_zero/yes"]] == 0x80000000).all()
    w = c.rows[c.groups["dense"], 0].view(F); k = out[c.groups["dense"]]
    fin = ~np.isnan(w); o = np.argsort(w[fin], kind="stable")
    assert (np.diff(k[fin][o].astype(np.int64)) >= 0).all()               # the key orders like the weight

    c = cases("n_is_convex"); out = hostprobe.run(c.fn, c.rows)[:, 0]
    assert (out[c.branches["n_is_convex.cos1>=cos2/yes"]] == 1).all() and (out[c.branches["n_is_convex.cos1>=cos2/no"]] == 0).all()

    for nm in ("a_tc", "a_tg"):
        c = cases(nm); out = hostprobe.run(c.fn, c.rows)
        cdf = c.rows[:, 4:].view(F)
        idx, bins = c.expect["top"]
        if nm == "a_tc":
            assert (out[idx, 1] == 0).all() and np.array_equal(out[idx, 0].view(F), cdf[idx, bins - 1] / F(2))      # bin == bins steps back
        else:
            assert (out[idx, 1] == ERR9).all()
        for k in ("err_low", "err_high"):
            assert (out[c.expect[k][0], 1] == ERR9).all() and (out[c.expect[k][0], 0] == 0).all(), (nm, k)
        idx, kk = c.expect["integral"]
        assert (out[idx, 1] == 0).all() and np.array_equal(out[idx, 0].view(F), cdf[idx, kk] / F(2)), nm
        assert (out[c.branches[nm + ".err/no"], 1] == 0).all()


# ---- the probe is the arithmetic the suite already trusts --------------------------------------------------------------------------
def _per_row(f, rows, n_in, n_out, restype=None):
    """an export that takes pointers to one row's floats: called row by row"""
    rows = np.ascontiguousarray(rows, np.uint32)
    out = np.zeros((len(rows), n_out), F)
    f.restype = restype
    if restype is None:
        f.argtypes = [VP, VP]
        a, o = rows.ctypes.data, out.ctypes.data
        for i in range(len(rows)):
            f(a + 4 * n_in * i, o + 4 * n_out * i)
    else:
        f.argtypes = [VP, VP]
        a = rows.ctypes.data
        res = [f(a + 24 * i, a + 24 * i + 12) for i in range(len(rows))]
        out[:, 0] = np.array(res, F)
    return out


@pytest.mark.parametrize("which", ["oracle", "emul"])
@pytest.mark.parametrize("name", ["n_ciede00", "n_rgb_eucl", "n_rgb2lab"])
def test_probe_equals_existing_exports(cases, hostprobe, oracle, emul, which, name):
    chk = oracle if which == "oracle" else emul
    c = cases(name)
    got = hostprobe.run(c.fn, c.rows).view(F)
    if name == "n_rgb2lab":
        want = _per_row(chk.fn("rgb2lab"), c.rows, 3, 3)
    else:
        want = _per_row(chk.fn("ciede00" if name == "n_ciede00" else "rgb_eucl"), c.rows, 6, 1, ctypes.c_float)
    bad = np.nonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all(1))[0]
    assert len(bad) == 0, "%d rows differ from %s; first: %s: %r vs %r" % (len(bad), which, c.describe(int(bad[0])), got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("which", ["oracle", "emul"])
def test_probe_equals_the_normal_export(hostprobe, oracle, emul, which):
    """n_plane_normal of the probe on the ordered sums == the `normal` export on the points (which sums them in the same order)"""
    chk = oracle if which == "oracle" else emul
    rng = np.random.default_rng(5)
    f = chk.fn("normal"); f.restype = None
    n = 0
    for k in (1, 2, 3, 4, 5, 9, 40, 300, 757):
        for transform in (False, True):
            pts = D._patches(rng, 400 if k <= 40 else 40, k, transform=transform)
            if k == 5:
                pts[::2, :, 2] = F(0.5)                  # exact planes
            if k == 4:
                pts[::2] = pts[::2, :1]                  # coincident
            rows = D.words(D.sums_f32(pts), np.full(len(pts), k, np.uint32), pts[:, 0, :])
            got = hostprobe.run(D.FN["n_plane_normal"], rows).view(F)
            want = np.zeros_like(got)
            for i in range(len(pts)):
                f(VP(pts[i].ctypes.data), ctypes.c_size_t(k), VP(pts[i, 0].ctypes.data), VP(want[i].ctypes.data))
            assert same_bits(got, want), (k, transform)
            n += len(pts)
    assert n > 5000


@pytest.mark.parametrize("name", [n for n in D.NAMES if D.FN[n] <= 10])
def test_probe_equals_oracle_math(cases, hostprobe, oracle, name):
    """ids 0..10 through literals and through a copy of the table == f3ds_oracle_math_vec"""
    c = cases(name)
    d = np.ascontiguousarray(c.rows).view(np.float64)
    a, b = np.ascontiguousarray(d[:, 0]), np.ascontiguousarray(d[:, 1])
    for off in (0, 100):
        want = np.empty_like(a)
        oracle.lib.f3ds_oracle_math_vec(c.fn + off, VP(a.ctypes.data), VP(b.ctypes.data), VP(want.ctypes.data), ctypes.c_size_t(len(a)))
        got = hostprobe.run(c.fn + off, c.rows).view(np.float64)[:, 0]
        assert same_bits(got, want), (name, off)


# ---- accuracy against plain float64 formulas (host side only: the device inherits it through bit equality) ------------------------------
def test_ciede2000_against_sharma_float64(cases, hostprobe):
    """n_ciede00 of the g++ probe against Sharma's formula in float64 numpy (degrees, hue mean by the paper's case distinction) on the
    dense rows: Lab of random, integer, grey and dark 8-bit colours through n_rgb2lab, unrelated and similar pairs.
    Measured maximum |difference|: 9.63e-6 (float32 result of values up to ~120; the float32 chroma sqrt(a*a + b*b) of the reference's
    formula is the rest).  Asserted: twice that."""
    c = cases("n_ciede00")
    idx = c.groups["dense"]
    got = hostprobe.run(c.fn, c.rows[idx]).view(F)[:, 0].astype(np.float64)
    f = c.rows[idx].view(F)
    want, _ = D.ciede2000_f64(f[:, :3], f[:, 3:])
    worst = float(np.abs(got - want).max())
    print("n_ciede00 vs float64 Sharma: max |d| = %.3g over %d rows" % (worst, len(idx)))
    assert worst <= 2 * 9.63e-6, worst


def test_voxel_distance_against_float64(cases, hostprobe):
    """n_voxel_distance of the g++ probe against the same formula in float64 numpy on the dense rows (centroids 0.3 - 12 m with and
    without the transform, unit and non-unit normals, seed resolutions 0.05 - 0.2, the default and random weights).
    Measured maximum relative difference |d| / max(1, |value|): 6.47e-7.  Asserted: twice that."""
    c = cases("n_voxel_distance")
    idx = c.groups["dense"]
    got = hostprobe.run(c.fn, c.rows[idx]).view(F)[:, 0].astype(np.float64)
    want = D.voxel_distance_f64(c.rows[idx])
    worst = float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())
    print("n_voxel_distance vs float64: max relative |d| = %.3g over %d rows" % (worst, len(idx)))
    assert worst <= 2 * 6.47e-7, worst


# ---- evl_scores ------------------------------------------------------------------------------------------------------------------
def test_evl_scores_equal_the_harness(hostprobe, harness):  # noqa: F811
    """evl_scores<evl_m_logf> with evl_visit_order / evl_match_column as the probe drives them == tests/eval_levels_harness, bit for bit"""
    tabs = evl_tables()
    got = hostprobe.evl(D.pack_tables([t[1:] for t in tabs]))
    for (what, table, ssize, tsize, N), g in zip(tabs, got):
        want = _harness_run(harness, table, ssize, tsize, N)[2]
        assert g.view(np.uint32).tolist() == want.view(np.uint32).tolist(), "%s: %r vs %r" % (what, g, want)


# ---- the build -------------------------------------------------------------------------------------------------------------------
def _make_lines():
    out = subprocess.run(["make", "-n", "-B", "-C", PROBE_DIR], check=True, capture_output=True, text=True).stdout
    return [l for l in out.splitlines() if "devprobe.hip" in l and "hipcc" in l]


def test_device_probe_is_compiled_with_the_products_flags():
    flags = subprocess.run(["make", "-s", "--no-print-directory", "-C", os.path.join(ROOT, "fast-3d-pointcloud-segmentation_amd", "csrc"), "print-flags"],
                           check=True, capture_output=True, text=True).stdout.split()
    assert "-ffp-contract=off" in flags and "--offload-arch=gfx950" in flags and len(flags) >= 5
    lines = _make_lines()
    assert len(lines) == 1, lines
    words = lines[0].split()
    for w in flags:
        assert w in words, "%s is missing from the probe's compile line: %s" % (w, lines[0])
    assert [w for w in words if w.startswith("-ffp-contract")] == ["-ffp-contract=off"]
    for bad in ("-ffast-math", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-fgpu-flush-denormals-to-zero", "-funsafe-math-optimizations", "-Ofast"):
        assert bad not in words, bad


def test_device_library_is_cross_compiled_for_gfx950(hostprobe):
    so = os.path.join(PROBE_DIR, "libf3ds_devprobe.so")
    assert os.path.exists(so)
    blob = open(so, "rb").read()
    assert b"gfx950" in blob and b"dp_rows" in blob and b"dp_normal_wave" in blob
    for sym in ("dp_dev_run", "dp_dev_ciede_quad", "dp_dev_edge_quad", "dp_dev_lab_three", "dp_dev_normal_wave", "dp_dev_evl"):
        assert sym.encode() in blob, sym
