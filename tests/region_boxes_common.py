"""Shared by tests/test_region_boxes_cpu.py and tests/test_region_boxes_gpu.py: the reference of the region boxes, written from the prose of
include/f3ds.h ("region boxes") and not from csrc/f3ds_boxes.h -- the shape rows from region_shapes_common.ref_shapes, points from
rgbd_common.numpy_deproject, the coordinate on the 2^-16 m grid, m, d and t as np.float32 operations written out one by one (each rounds once), minima and maxima on key-ordered
u32 views, the residual sum as a Python integer.  Rows are compared bit for bit as 24 u32 words: empty rows hold NaN."""
import numpy as np

import region_shapes_common as S
import region_table_common as R
from region_table_common import NO, QNAN
from rgbd_common import numpy_deproject

u32, f32, f64 = np.uint32, np.float32, np.float64
RESULT_FIELDS = ("n_regions", "n_nonempty", "n_labelled", "n_clamped", "n_inliers")
EMPTY_ROW = np.array([0, 0] + [QNAN] * 22, u32)
TOL = 0.01      # the package's default plane_tol


def grid_f32(a):
    """q: the coordinate clamped to +-32768 (a NaN to -32768), rounded to units of 2^-16 m as the table's fixed point, and converted to f32 once"""
    a = np.asarray(a, f32).astype(f64)
    with np.errstate(invalid="ignore"):
        d = np.where(a >= -32768.0, a, -32768.0)      # (NaN too)
        d = np.where(d > 32768.0, 32768.0, d)
    return (np.rint(d * 65536.0) * 2.0 ** -16).astype(f32)


def canon(t):
    """the bits of t, a NaN as 0x7FC00000"""
    t = np.asarray(t, f32)
    return np.where(t != t, u32(QNAN), t.view(u32)).astype(u32)


def cross_f32(n, l):
    """m = n x l: two rounded f32 products and one rounded f32 subtraction a component"""
    n, l = [f32(x) for x in n], [f32(x) for x in l]
    return [f32(f32(n[1] * l[2]) - f32(n[2] * l[1])), f32(f32(n[2] * l[0]) - f32(n[0] * l[2])), f32(f32(n[0] * l[1]) - f32(n[1] * l[0]))]


def project(q, c, e):
    """t_e = (d_x * e_x + d_y * e_y) + d_z * e_z of the points q (k x 3 f32) about c, every operation one rounded f32 operation"""
    d = [(q[:, a] - f32(c[a])).astype(f32) for a in range(3)]
    p = [(d[a] * f32(e[a])).astype(f32) for a in range(3)]
    return ((p[0] + p[1]).astype(f32) + p[2]).astype(f32)


def frame_of(shape_row):
    """(c, (n, m, l)) from the public floats of a shape row"""
    c = [f32(x) for x in shape_row["centroid"]]
    n = [f32(x) for x in shape_row["normal"]]
    l = [f32(x) for x in shape_row["axis"]]
    return c, (n, cross_f32(n, l), l)


def labelled_points(fmt, depth, labels):
    """(pixel indices, labels, q (k x 3 f32)) of the labelled pixels"""
    h, w = int(fmt.height), int(fmt.width)
    lab = np.asarray(labels, u32).reshape(-1)
    pts = numpy_deproject(fmt, depth, np.zeros((h, w), u32))
    p = np.flatnonzero(~np.isnan(pts[:, 2]) & (lab != NO))
    return p, lab[p], grid_f32(np.ascontiguousarray(pts[p, :3]))


def ref_boxes(P, fmt, depth, labels, n_regions, plane_tol=TOL):
    """(rc, rows (REGION_BOX_DTYPE), shapes (REGION_SHAPE_DTYPE), result dict) of the definition; the last three are None unless rc == 0"""
    K = int(n_regions)
    rc, shapes, sres, _ = S.ref_shapes(P, fmt, depth, labels, K)
    if rc:
        return rc, None, None, None
    _, lab, q = labelled_points(fmt, depth, labels)
    tol = f32(plane_tol)
    words = np.tile(EMPTY_ROW, (K, 1))
    total_inliers = 0
    half = f32(0.5)
    with np.errstate(all="ignore"):
        for r in np.unique(lab).tolist():
            sel = lab == r
            c, axes = frame_of(shapes[r])
            t = [project(q[sel], c, e) for e in axes]
            keys = [R.key(canon(x)) for x in t]
            lo = np.array([R.unkey(k.min()) for k in keys], u32).view(f32)
            hi = np.array([R.unkey(k.max()) for k in keys], u32).view(f32)
            res = np.abs(t[0]).astype(f32)
            inl = int((res <= tol).sum())
            a = res.astype(f64)
            a = np.where(a >= -32768.0, a, -32768.0)      # (NaN too)
            a = np.where(a > 32768.0, 32768.0, a)
            total = sum(np.rint(a * 65536.0).astype(np.int64).tolist())      # a Python integer
            n = int(sel.sum())
            hf = [f32(f32(hi[k] - lo[k]) * half) for k in range(3)]
            mid = [f32(f32(lo[k] + hi[k]) * half) for k in range(3)]
            center = [f32(f32(f32(c[a_] + f32(mid[0] * axes[0][a_])) + f32(mid[1] * axes[1][a_])) + f32(mid[2] * axes[2][a_])) for a_ in range(3)]
            mean = f32((float(total) / float(n)) * 2.0 ** -16)
            floats = center + axes[0] + axes[1] + axes[2] + list(lo) + list(hi) + hf + [mean]
            words[r, 0], words[r, 1] = n, inl
            words[r, 2:] = np.array(floats, f32).view(u32)
            total_inliers += inl
    rows = np.ascontiguousarray(words).reshape(-1).view(P.REGION_BOX_DTYPE)
    return R.OK, rows, shapes, dict(sres, n_inliers=total_inliers)


_refs = {}


def reference(P, key, sc, plane_tol=TOL):
    """the reference of a scene, computed once per key and tolerance and left unchanged"""
    k = (key, float(plane_tol))
    if k not in _refs:
        _refs[k] = ref_boxes(P, sc["fmt"], sc["depth"], sc["labels"], sc["n_regions"], plane_tol)
    return _refs[k]


def words_of(rows):
    return np.ascontiguousarray(rows).view(u32).reshape(len(rows), 24)


def assert_rows_equal(P, got, want, what=""):
    g, w = words_of(got), words_of(want)
    if not np.array_equal(g, w):
        i, k = [int(a[0]) for a in np.nonzero(g != w)]
        raise AssertionError("%s row %d word %d: %#x, want %#x\ngot  %r\nwant %r" % (what, i, k, g[i, k], w[i, k], got[i], want[i]))


def assert_contained(rows, shapes, fmt, depth, labels):
    """every labelled pixel's t, recomputed about the shape row's centroid along the axes the BOX row holds, lies in [lo, hi] of its region's row in key
    order, exactly, and both ends are met"""
    _, lab, q = labelled_points(fmt, depth, labels)
    seen = 0
    for r in np.unique(lab).tolist():
        row, sel = rows[r], lab == r
        assert int(sel.sum()) == int(row["n_pixels"])
        c = [f32(x) for x in shapes[r]["centroid"]]
        for k, name in enumerate(("axis_n", "axis_m", "axis_l")):
            keys = R.key(canon(project(q[sel], c, [f32(x) for x in row[name]])))
            lo, hi = R.key(row["lo"][k:k + 1].view(u32))[0], R.key(row["hi"][k:k + 1].view(u32))[0]
            assert lo <= keys.min() and keys.max() <= hi, (r, name)
            assert lo == keys.min() and hi == keys.max(), (r, name)
        seen += int(sel.sum())
    return seen
