"""Shared by tests/test_cloud_regions_cpu.py, tests/test_cloud_regions_gpu.py and tests/test_cloud_regions_batch_gpu.py: the reference of the region rows of a
point cloud, written from the prose of include/f3ds.h ("region rows of a point cloud") and not from csrc/f3ds_cloud.h -- the fold and the finiteness test on
np.float32, the fixed point with np.rint on f64, n, S, M and the colour sums as Python integers of unbounded size, the twenty shape floats from
region_shapes_common.shape_row (Jacobi on Python floats), minima and maxima on key-ordered u32 views, the boxes with the f32 helpers of region_boxes_common --
and the clouds all three files run.  Rows are compared bit for bit as 32 u32 words: empty rows hold NaN."""
import ctypes

import numpy as np

import region_boxes_common as B
import region_shapes_common as S
import region_table_common as R
from region_table_common import NO, QNAN

u32, f32, f64 = np.uint32, np.float32, np.float64
RESULT_FIELDS = ("n_regions", "n_nonempty", "n_labelled", "n_clamped", "n_inliers")
POS_INF, NEG_INF = 0x7F800000, 0xFF800000
EMPTY_ROW = np.array([0, NO] + [POS_INF] * 3 + [NEG_INF] * 3 + [QNAN] * 23 + [0], u32)
TOL = 0.01
ERR_LOGIC = -5


def records(xyz, rgba=None):
    """(n, 4) f32 records from (n, 3) coordinates and n colour words"""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    pts = np.zeros((len(xyz), 4), f32)
    pts[:, :3] = xyz
    if rgba is not None:
        pts[:, 3] = np.asarray(rgba, u32).view(f32)
    return pts


def labelled_points(pts, labels, fold):
    """(indices, labels, xyz (k x 3 f32, after the fold), colour words) of the labelled points"""
    pts = np.asarray(pts, f32).reshape(-1, 4)
    lab = np.asarray(labels, u32).reshape(-1)
    xyz = pts[:, :3].copy()
    if fold:
        z = xyz[:, 2]
        with np.errstate(invalid="ignore"):
            xyz[:, 2] = np.where(z < 0, np.abs(z), z)
    i = np.flatnonzero(np.isfinite(xyz).all(axis=1) & (lab != NO))
    return i, lab[i], np.ascontiguousarray(xyz[i]), np.ascontiguousarray(pts[:, 3]).view(u32)[i]


def ref_cloud(P, pts, labels, n_regions, plane_tol=TOL, fold=0, want_boxes=True):
    """(rc, rows (CLOUD_REGION_DTYPE), boxes (REGION_BOX_DTYPE) or None, result dict) of the definition; the last three are None unless rc == 0"""
    K = int(n_regions)
    lab_all = np.asarray(labels, u32).reshape(-1)
    if ((lab_all != NO) & (lab_all >= K)).any():
        return R.ERR_ARG, None, None, None
    idx, lab, xyz, rgba = labelled_points(pts, labels, fold)
    a = xyz.astype(f64)
    cl = np.clip(a, -32768.0, 32768.0)
    clamped = (cl != a).any(axis=1)
    fix = np.rint(cl * 65536.0).astype(np.int64)
    keys = R.key(xyz.view(u32))
    words = np.tile(EMPTY_ROW, (K, 1))
    bwords = np.tile(B.EMPTY_ROW, (K, 1))
    tol, half, total_inliers = f32(plane_tol), f32(0.5), 0
    order = np.argsort(lab, kind="stable")
    cuts = np.flatnonzero(np.diff(lab[order])) + 1
    with np.errstate(all="ignore"):
        for sel in np.split(order, cuts) if len(order) else []:
            r, n = int(lab[sel[0]]), len(sel)
            f = fix[sel].tolist()
            Ssum = [sum(p[k] for p in f) for k in range(3)]
            M = [sum(p[i] * p[j] for p in f) for i, j in S.PAIRS]
            floats, _ = S.shape_row(n, Ssum, M)      # centroid 3, cov 6, eigenvalue 3, normal 3, axis 3, plane_d, curvature
            c = rgba[sel].astype(np.int64)
            rgb = [f32(float(int(((c >> s) & 255).sum())) / float(n)) for s in (16, 8, 0)]
            lo, hi = R.unkey(keys[sel].min(axis=0)), R.unkey(keys[sel].max(axis=0))
            words[r, 0], words[r, 1] = n, int(idx[sel].min())
            words[r, 2:5], words[r, 5:8] = lo, hi
            words[r, 8:11] = np.array(floats[0:3], f32).view(u32)
            words[r, 11:14] = np.array(rgb, f32).view(u32)
            words[r, 14:31] = np.array(floats[3:], f32).view(u32)
            if not want_boxes:
                continue
            cen, nrm, axl = floats[0:3], floats[12:15], floats[15:18]
            axes = (nrm, B.cross_f32(nrm, axl), axl)
            q = B.grid_f32(xyz[sel])
            t = [B.project(q, cen, e) for e in axes]
            tk = [R.key(B.canon(x)) for x in t]
            blo = np.array([R.unkey(k.min()) for k in tk], u32).view(f32)
            bhi = np.array([R.unkey(k.max()) for k in tk], u32).view(f32)
            res = np.abs(t[0]).astype(f32)
            inl = int((res <= tol).sum())
            ra = np.clip(res.astype(f64), -32768.0, 32768.0)
            total = sum(np.rint(ra * 65536.0).astype(np.int64).tolist())
            hf = [f32(f32(bhi[k] - blo[k]) * half) for k in range(3)]
            mid = [f32(f32(blo[k] + bhi[k]) * half) for k in range(3)]
            center = [f32(f32(f32(cen[a_] + f32(mid[0] * axes[0][a_])) + f32(mid[1] * axes[1][a_])) + f32(mid[2] * axes[2][a_])) for a_ in range(3)]
            mean = f32((float(total) / float(n)) * 2.0 ** -16)
            bwords[r, 0], bwords[r, 1] = n, inl
            bwords[r, 2:] = np.array(center + list(axes[0]) + list(axes[1]) + list(axes[2]) + list(blo) + list(bhi) + hf + [mean], f32).view(u32)
            total_inliers += inl
    rows = np.ascontiguousarray(words).reshape(-1).view(P.CLOUD_REGION_DTYPE)
    boxes = np.ascontiguousarray(bwords).reshape(-1).view(P.REGION_BOX_DTYPE) if want_boxes else None
    result = dict(n_regions=K, n_nonempty=len(np.unique(lab)), n_labelled=int(len(idx)), n_clamped=int(clamped.sum()), n_inliers=total_inliers)
    return R.OK, rows, boxes, result


_refs = {}


def reference(P, name):
    """the reference of a named cloud (CLOUDS), with boxes, computed once and left unchanged"""
    if name not in _refs:
        c = cloud(name)
        _refs[name] = ref_cloud(P, c["pts"], c["labels"], c["K"], c["tol"], c["fold"])
    return _refs[name]


def words_of(rows):
    return np.ascontiguousarray(rows).view(u32).reshape(len(rows), 32)


def assert_rows_equal(got, want, what=""):
    g, w = words_of(got), words_of(want)
    if not np.array_equal(g, w):
        i, k = [int(a[0]) for a in np.nonzero(g != w)]
        raise AssertionError("%s row %d word %d: %#x, want %#x\ngot  %r\nwant %r" % (what, i, k, g[i, k], w[i, k], got[i], want[i]))


def params_of(P, tol=TOL, fold=0):
    return P.CloudParams(float(tol), int(fold))


def c_cloud(P, pts, labels, n_regions, tol=TOL, fold=0, want_boxes=True, fill=0xA5):
    """f3ds_cloud_regions_host on raw buffers: (rc, rows, boxes, result); rows and boxes prefilled with `fill` bytes, the result with sevens"""
    lib = P.load_library()
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 4)
    lab = np.ascontiguousarray(labels, u32).reshape(-1)
    K = int(n_regions)
    rows = np.frombuffer(bytes([fill]) * (128 * K), P.CLOUD_REGION_DTYPE).copy()
    boxes = np.frombuffer(bytes([fill]) * (96 * K), P.REGION_BOX_DTYPE).copy()
    res = P.CloudRegionsResult(7, 7, 7, 7, 7)
    spare = np.zeros(4, f32)
    prm = params_of(P, tol, fold)
    rc = lib.f3ds_cloud_regions_host(pts.ctypes.data if len(pts) else spare.ctypes.data, len(lab), lab.ctypes.data if len(lab) else spare.ctypes.data, K, ctypes.byref(prm),
                                     rows.ctypes.data if K else None, boxes.ctypes.data if K and want_boxes else None, ctypes.byref(res))
    return rc, rows, boxes, res


# ---- the clouds ---------------------------------------------------------------------------------------------------------------------------------------------
def patches(n, K, seed, scatter=True):
    """n points on K tilted planar patches with a little noise, a colour per point; labels scattered by a fixed permutation (or in runs, label by label)"""
    rng = np.random.default_rng(seed)
    lab = (np.arange(n) * K // max(n, 1)).astype(u32) if n else np.zeros(0, u32)      # every label gets its share, in runs
    centre = rng.uniform(-2.0, 2.0, (K, 3)) + np.array([0.0, 0.0, 3.0])
    e1, e2 = rng.normal(size=(K, 3)), rng.normal(size=(K, 3))
    uv = rng.uniform(-0.3, 0.3, (n, 2))
    xyz = centre[lab] + uv[:, :1] * e1[lab] + uv[:, 1:] * 0.3 * e2[lab] + rng.normal(scale=0.002, size=(n, 3))
    rgba = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(u32)
    pts = records(xyz, rgba)
    if scatter and n:
        perm = np.random.default_rng(seed + 1).permutation(n)
        pts, lab = np.ascontiguousarray(pts[perm]), np.ascontiguousarray(lab[perm])
    return pts, lab


def _edge(name):
    nan, inf = np.nan, np.inf
    if name == "one_coordinate_not_finite":      # NaN or +-inf in exactly one coordinate: six points out, the rest in
        pts, lab = patches(40, 3, 31)
        for k, (col, v) in enumerate(((0, nan), (1, nan), (2, nan), (0, inf), (1, -inf), (2, inf))):
            pts[5 * k + 1, col] = v
        return pts, lab, 3
    if name == "signed_zero":                    # -0.0 against +0.0: lo is -0, hi is +0
        xyz = [[-0.0, 0.0, 1.0], [0.0, -0.0, 1.0], [0.0, 0.0, 1.0], [-0.0, -0.0, 1.0], [0.0, 1.0, -0.0], [-0.0, 2.0, 0.0]]
        return records(xyz, np.arange(6) * 0x010203), np.array([0, 0, 0, 0, 1, 1], u32), 2
    if name == "clamped":                        # coordinates beyond +-32768: clamped, counted, and lo / hi keep the raw floats
        xyz = [[40000.0, 1.0, 2.0], [-50000.0, 1.0, 2.5], [3.0e38, -3.0e38, 32768.0], [1.0, 2.0, 3.0], [32768.5, -32768.5, 1.0], [2.0, 2.0, 2.0], [2.0, 2.5, 2.0]]
        return records(xyz, np.arange(7) * 77), np.array([0, 0, 0, 0, 1, 1, 1], u32), 2
    if name == "no_label_over_finite":           # F3DS_NO_LABEL over finite points; region 2 gets no point at all
        pts, lab = patches(60, 2, 37)
        lab[::3] = NO
        return pts, lab, 3
    if name == "labels_over_not_finite":         # labels over non-finite points: region 1 has nothing else
        pts, lab = patches(30, 1, 41)
        extra = records([[nan, 0, 1], [0, inf, 1], [1, 1, -inf], [nan, nan, nan]], [1, 2, 3, 4])
        return np.concatenate([pts, extra]), np.concatenate([lab, np.array([1, 1, 1, 0], u32)]), 2
    raise ValueError(name)


CLOUDS = ["empty", "one_point", "one_region", "K23", "K200", "K3000", "one_coordinate_not_finite", "signed_zero", "clamped", "negative_z", "negative_z_folded",
          "no_label_over_finite", "labels_over_not_finite"]
LAUNCH_SIZES = [63, 64, 65, 257, 769]      # around a wave, one point more than a workgroup, one more than three workgroups (a span each at width 3)
_clouds = {}


def cloud(name):
    """dict(pts, labels, K, tol, fold) of a named cloud, built once"""
    if name in _clouds:
        return _clouds[name]
    tol, fold = TOL, 0
    if name == "empty":
        pts, lab, K = np.zeros((0, 4), f32), np.zeros(0, u32), 4
    elif name == "one_point":
        pts, lab, K = records([[0.25, -1.5, 2.0]], [0x00804020]), np.array([1], u32), 2
    elif name == "one_region":
        pts, lab = patches(500, 1, 11)
        K = 1
    elif name in ("K23", "K200", "K3000"):
        K = int(name[1:])
        pts, lab = patches(6000, K, 13 + K)
    elif name in ("negative_z", "negative_z_folded"):
        pts, lab = patches(300, 4, 17)
        pts[::2, 2] = -pts[::2, 2]
        pts[7, 2] = -np.inf      # folds to +inf: not finite either way
        K, fold = 4, int(name.endswith("folded"))
    elif name[:1] == "n" and name[1:].isdigit():      # "n65": that many points on five patches, scattered
        n = int(name[1:])
        pts, lab = patches(n, 5, 100 + n)
        K = 5
    else:
        pts, lab, K = _edge(name)
    _clouds[name] = dict(pts=pts, labels=lab, K=K, tol=tol, fold=fold)
    return _clouds[name]


# ---- the image scenes as clouds -----------------------------------------------------------------------------------------------------------------------------
def scene_cloud(P, which, width, height, depth_kind):
    """(scene dict with the rgb8 format and a colour image, records of f3ds_deproject) of a scene of the region table / the region shapes"""
    sc = S.any_scene(P, which, width, height, depth_kind)
    fmt = R.with_color(P, sc["fmt"], "rgb8")
    color = R.make_color(width, height, "rgb8")
    return dict(sc, fmt=fmt, color=color), P.deproject(fmt, sc["depth"], color)
