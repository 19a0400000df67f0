"""Shared by tests/test_region_shapes_cpu.py and tests/test_region_shapes_gpu.py: the reference of the region shapes, written from the prose of
include/f3ds.h ("region shapes") and not from csrc/f3ds_shapes.h -- points from rgbd_common.numpy_deproject, the table's fixed point, n, S and M as Python
integers of unbounded size (no split halves), N exactly, float(N) for the one rounding (Python's int -> float conversion rounds to nearest even), Jacobi on
Python floats with math.sqrt, np.float32(...) for the last step -- and the scenes both files add to those of tests/region_table_common.py.  Rows are
compared bit for bit as u32 words: empty rows hold NaN."""
import math

import numpy as np

import region_table_common as R
from region_table_common import NO, QNAN
from rgbd_common import frame_format, numpy_deproject

u32, f32, f64 = np.uint32, np.float32, np.float64
RESULT_FIELDS = ("n_regions", "n_nonempty", "n_labelled", "n_clamped")
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # xx, xy, xz, yy, yz, zz
SWEEPS = 8
EXTRA = ["8+2", "tilted", "flat", "thin", "mirror"]


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------
def jacobi(C):
    """(C, V) after exactly 8 cyclic sweeps; C: 3 x 3 list of Python floats, changed in place"""
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = C[p][q]
            if apq == 0.0:
                continue
            r = 3 - p - q
            theta = (C[q][q] - C[p][p]) / (2.0 * apq)
            t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
            if theta < 0:
                t = -t
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            C[p][p] -= t * apq
            C[q][q] += t * apq
            C[p][q] = C[q][p] = 0.0
            arp, arq = C[r][p], C[r][q]
            C[r][p] = C[p][r] = c * arp - s * arq
            C[r][q] = C[q][r] = s * arp + c * arq
            for k in range(3):
                vp, vq = V[k][p], V[k][q]
                V[k][p] = c * vp - s * vq
                V[k][q] = s * vp + c * vq
    return C, V


def shape_row(n, S, M):
    """the twenty floats of a non-empty region from its exact integers, as np.float32, and the f64 covariance"""
    cen = [(float(S[a]) / float(n)) * 2.0 ** -16 for a in range(3)]
    cov = [((float(n * M[k] - S[a] * S[b]) / float(n)) / float(n)) * 2.0 ** -32 for k, (a, b) in enumerate(PAIRS)]
    C = [[cov[0], cov[1], cov[2]], [cov[1], cov[3], cov[4]], [cov[2], cov[4], cov[5]]]
    C, V = jacobi(C)
    lam = [C[k][k] if not C[k][k] < 0 else 0.0 for k in range(3)]
    order = sorted(range(3), key=lambda k: lam[k])      # (stable: ties by column index)
    lam = [lam[k] for k in order]
    v = [V[k][order[0]] for k in range(3)]
    d = (v[0] * cen[0] + v[1] * cen[1]) + v[2] * cen[2]
    if d > 0:
        v, d = [-x for x in v], -d
    w = [V[k][order[2]] for k in range(3)]
    big = 0
    for k in (1, 2):
        if abs(w[k]) > abs(w[big]):
            big = k
    if w[big] < 0:
        w = [-x for x in w]
    total = (lam[0] + lam[1]) + lam[2]
    curv = f32(lam[0] / total) if total > 0 else f32(0.0)
    return [f32(x) for x in cen + cov + lam + v + w + [-d]] + [curv], cov


def ref_shapes(P, fmt, depth, labels, n_regions):
    """(rc, rows (REGION_SHAPE_DTYPE), result dict, moments) of the definition; the last three are None unless rc == 0.  moments: per non-empty region
    (n, S, M) as Python integers and the f64 covariance."""
    h, w = int(fmt.height), int(fmt.width)
    K = int(n_regions)
    lab = np.asarray(labels, u32).reshape(-1)
    if ((lab != NO) & (lab >= K)).any():
        return R.ERR_ARG, None, None, None
    pts = numpy_deproject(fmt, depth, np.zeros((h, w), u32))
    p = np.flatnonzero(~np.isnan(pts[:, 2]) & (lab != NO))
    a = np.ascontiguousarray(pts[p, :3]).astype(f64)
    cl = np.clip(a, -32768.0, 32768.0)
    clamped = (cl != a).any(axis=1)
    fix = np.rint(cl * 65536.0).astype(np.int64).tolist()
    sums = {}
    for r, f in zip(lab[p].tolist(), fix):
        e = sums.get(r)
        if e is None:
            e = sums[r] = [0, [0, 0, 0], [0] * 6]
        e[0] += 1
        for k in range(3):
            e[1][k] += f[k]
        for k, (i, j) in enumerate(PAIRS):
            e[2][k] += f[i] * f[j]
    words = np.full((K, 21), QNAN, u32)
    words[:, 0] = 0
    moments = {}
    for r, (n, S, M) in sums.items():
        floats, cov = shape_row(n, S, M)
        words[r, 0] = n
        words[r, 1:] = np.array(floats, f32).view(u32)
        moments[r] = (n, S, M, cov)
    rows = words.reshape(-1).view(P.REGION_SHAPE_DTYPE)
    return R.OK, rows, dict(n_regions=K, n_nonempty=len(sums), n_labelled=int(len(p)), n_clamped=int(clamped.sum())), moments


_refs = {}


def reference(P, key, sc):
    """the reference of a scene, computed once per key ((scene, width, height, depth kind) or any other hashable) and left unchanged"""
    if key not in _refs:
        _refs[key] = ref_shapes(P, sc["fmt"], sc["depth"], sc["labels"], sc["n_regions"])
    return _refs[key]


def words_of(rows):
    return np.ascontiguousarray(rows).view(u32).reshape(len(rows), 21)


def assert_rows_equal(P, got, want, what=""):
    g, w = words_of(got), words_of(want)
    if not np.array_equal(g, w):
        i, k = [int(a[0]) for a in np.nonzero(g != w)]
        raise AssertionError("%s row %d word %d: %#x, want %#x\ngot  %r\nwant %r" % (what, i, k, g[i, k], w[i, k], got[i], want[i]))


# ---- the scenes this feature adds ---------------------------------------------------------------------------------------------------------------------------
def extra_scene(P, which, width, height, depth_kind):
    """"8+2"    scene 8's images (depth_scale 4: z clamped at 32768 m, every f_z^2 = 2^62) under scene 2's labels (one region): M_zz leaves 64 bits
    "tilted" (a) one region on a plane n . p = 1 that faces the camera obliquely: 1 / z linear in (u, v), f32 depths
    "flat"   (a) one region at one constant f32 depth, fronto-parallel
    "thin"   (b) region 0 is one pixel wide (a column whose points lie on a line oblique to all three axes), region 1 is one pixel, region 2 two pixels
             of one row at one depth, region 3 the rest
    "mirror" (c) two regions with the same geometry mirrored in x: the left and the right half of a symmetric roof"""
    w, h = width, height
    if which == "8+2":
        sc = R.scene(P, 8, w, h, depth_kind)
        return dict(sc, labels=np.zeros((h, w), u32), n_regions=1)
    fmt = frame_format(P, w, h, "f32", "rgb8", 1.0)
    uu, vv = np.meshgrid(np.arange(w, dtype=f64), np.arange(h, dtype=f64))
    if which == "tilted":
        inv = 0.5 + 0.2 * (uu - fmt.cx) / fmt.fx - 0.1 * (vv - fmt.cy) / fmt.fy      # n = (0.2, -0.1, 0.5): z = 1 / (n . ray)
        return dict(fmt=fmt, depth=(1.0 / inv).astype(f32), labels=np.zeros((h, w), u32), n_regions=1)
    if which == "flat":
        return dict(fmt=fmt, depth=np.full((h, w), 1.7, f32), labels=np.zeros((h, w), u32), n_regions=1)
    if which == "thin":
        lab = np.full((h, w), 3, u32)
        lab[:, w // 3] = 0
        lab[0, 0] = 1
        depth = (1.0 / (0.5 - 0.1 * (vv - fmt.cy) / fmt.fy)).astype(f32)      # a plane tilted about x: the column's points lie on a line through x, y and z
        depth[h - 1, :] = f32(2.0)
        lab[h - 1, :] = NO      # (the last row is off the plane)
        lab[h - 1, 0:2] = 2
        return dict(fmt=fmt, depth=depth, labels=lab, n_regions=4)
    if which == "mirror":
        fmt.cx = (w - 1) / 2.0
        lab = (uu > (w - 1) / 2.0).astype(u32)
        if w % 2:
            lab[:, w // 2] = NO      # the centre column belongs to neither half
        depth = (2.0 - 0.5 * np.abs(uu - (w - 1) / 2.0) / w + 0.002 * vv).astype(f32)
        return dict(fmt=fmt, depth=depth, labels=lab.astype(u32), n_regions=2)
    raise ValueError(which)


def any_scene(P, which, width, height, depth_kind):
    return extra_scene(P, which, width, height, depth_kind) if isinstance(which, str) else R.scene(P, which, width, height, depth_kind)


# ---- properties, in f64 from the f32 rows -----------------------------------------------------------------------------------------------------------------
def properties(rows, moments):
    """what holds for every non-empty row of a converged decomposition; moments: the reference's (ref_shapes), for the f64 covariance.  The bounds: a unit
    vector rounded to f32 is within 2^-22 of length 1; the residual of the f32-rounded outputs measures 2^-24 of the largest eigenvalue after four sweeps, so
    2^-20 leaves sixteen f32 roundings; the eigenvalues carry one f32 rounding (2^-24) against those of the f64 covariance."""
    for r in np.flatnonzero(rows["n_pixels"] > 0):
        row = rows[r]
        lam = row["eigenvalue"].astype(f64)
        assert lam[0] >= 0 and lam[0] <= lam[1] <= lam[2], lam
        n, a, cen = row["normal"].astype(f64), row["axis"].astype(f64), row["centroid"].astype(f64)
        assert abs(np.linalg.norm(n) - 1) <= 2.0 ** -22 and abs(np.linalg.norm(a) - 1) <= 2.0 ** -22, (np.linalg.norm(n), np.linalg.norm(a))
        assert float(n @ cen) <= 0 and row["plane_d"] >= 0
        c = row["cov"].astype(f64)
        C = np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])
        for v, l in ((n, lam[0]), (a, lam[2])):
            assert np.abs(C @ v - l * v).max() <= 2.0 ** -20 * lam[2], (int(r), np.abs(C @ v - l * v).max(), lam)
        c = moments[int(r)][3]
        C = np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])
        assert np.abs(np.linalg.eigvalsh(C) - lam).max() <= 2.0 ** -22 * lam[2], (int(r), np.linalg.eigvalsh(C), lam)
