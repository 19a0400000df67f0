"""Shared by tests/test_region_joints_cpu.py and tests/test_region_joints_gpu.py: the reference of the region joints, written from the prose of
include/f3ds.h ("region joints") and not from csrc/f3ds_joints.h -- the contact pairs from region_contacts_common.pairs_of, the shape rows from
region_shapes_common.ref_shapes, the samples' n, S and M as Python integers of unbounded size, their finish by region_shapes_common.shape_row, the join as
np.float32 operations written out one by one (each rounds once).  The reference does not call the library.  Rows are compared bit for bit as 20 u32
words.  The last section is the GPU test's: the device call on raw buffers against f3ds_region_joints_host, which the CPU test holds against the reference.

Scenes: the contacts' 1 ... 10 (region_contacts_common.scene) and the analytic ones of analytic_scene(): exact planes by ray-plane intersection at 64 x 48,
fx = fy = 60, the left half label 0 and the right half label 1, the border on x = 0."""
import numpy as np

import region_contacts_common as C
import region_shapes_common as S
import region_table_common as R
from region_table_common import NO, QNAN
from rgbd_common import frame_format, numpy_deproject

u32, f32, f64 = np.uint32, np.float32, np.float64
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_CAPACITY = C.OK, C.ERR_ARG, C.ERR_UNSUPPORTED, C.ERR_CAPACITY
OCCLUSION, COPLANAR, CONVEX, CONCAVE, REF_CONVEX = 0, 1, 2, 3, 0x100
DEFAULTS = (0.05, 0.01, 0.9659258)      # depth_tol, plane_tol, cos_coplanar
RESULT_FIELDS = ("n_regions", "n_joints", "n_surface", "reserved", "n_pairs", "n_close")
SCENES = C.SCENES
SHAPES = C.SHAPES
ANALYTIC = {"ridge": CONVEX, "valley": CONCAVE, "one_plane": COPLANAR, "plate": OCCLUSION}
buffers = R.buffers


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------
def sum3(a, b, c):
    """the reference's three-term sum: a + (b + c), two rounded f32 adds"""
    return (a + (b + c).astype(f32)).astype(f32)


def dot3(n, c):
    """(n_x * c_x + n_y * c_y) + n_z * c_z on k x 3 f32 arrays, every operation one rounded f32 operation"""
    p = [(n[:, k] * c[:, k]).astype(f32) for k in range(3)]
    return ((p[0] + p[1]).astype(f32) + p[2]).astype(f32)


def plane(n, c, d):
    return (dot3(n, c) + d).astype(f32)


def unit_c(c1, c2):
    C_ = [(c1[:, k] - c2[:, k]).astype(f32) for k in range(3)]
    n = np.sqrt(sum3(*[(x * x).astype(f32) for x in C_])).astype(f32)
    return [(x / n).astype(f32) for x in C_]


def normals_diff(n1, c1, n2, c2):
    """(delta_g, is_convex) of the reference's Clustering::normals_diff / is_convex on k x 3 f32 arrays"""
    C_ = unit_c(c1, c2)
    cr = [((n1[:, i] * n2[:, j]).astype(f32) - (n1[:, j] * n2[:, i]).astype(f32)).astype(f32) for i, j in ((1, 2), (2, 0), (0, 1))]
    nxn = np.sqrt(sum3(*[(x * x).astype(f32) for x in cr])).astype(f32)
    cos1 = sum3(*[(n1[:, k] * C_[k]).astype(f32) for k in range(3)])
    cos2 = sum3(*[(n2[:, k] * C_[k]).astype(f32) for k in range(3)])
    g = (((nxn + np.abs(cos1)).astype(f32) + np.abs(cos2)).astype(f32) / f32(3)).astype(f32)
    return g, cos1 >= cos2


def canon(t):
    t = np.asarray(t, f32)
    return np.where(t != t, u32(QNAN), t.view(u32)).astype(u32)


def ref_joints(P, fmt, depth, labels, n_regions, prm=DEFAULTS):
    """(rc, rows (REGION_JOINT_DTYPE), shapes (REGION_SHAPE_DTYPE), result dict) of the definition; the last three are None unless rc == 0"""
    K = int(n_regions)
    h, w = int(fmt.height), int(fmt.width)
    depth_tol, plane_tol, cos_coplanar = [f32(x) for x in prm]
    rc, shapes, _, _ = S.ref_shapes(P, fmt, depth, labels, K)
    if rc:
        return rc, None, None, None
    c = C.pairs_of(fmt, depth, labels, depth_tol)
    ab = np.stack([c["a"], c["b"]], axis=1)
    uniq, inv = np.unique(ab, axis=0, return_inverse=True) if len(ab) else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    inv = np.asarray(inv).reshape(-1)
    J = len(uniq)
    n_pairs = np.bincount(inv, minlength=J).astype(np.int64)
    n_close = np.bincount(inv, weights=c["close"].astype(f64), minlength=J).astype(np.int64)
    # the samples: both points of every close pair, fixed as the table does, summed as Python integers
    pts = numpy_deproject(fmt, depth, np.zeros((h, w), u32))[:, :3]
    a64 = np.ascontiguousarray(pts).astype(f64)
    with np.errstate(invalid="ignore"):
        fix = np.rint(np.clip(np.where(np.isnan(a64), -32768.0, a64), -32768.0, 32768.0) * 65536.0).astype(np.int64)
    sums = [[0, [0, 0, 0], [0] * 6] for _ in range(J)]
    for e, p, q in zip(inv[c["close"]].tolist(), c["p"][c["close"]].tolist(), c["q"][c["close"]].tolist()):
        for x in (p, q):
            f = fix[x].tolist()
            sums[e][0] += 1
            for k in range(3):
                sums[e][1][k] += f[k]
            for k, (i, j) in enumerate(S.PAIRS):
                sums[e][2][k] += f[i] * f[j]
    cen, direction, spread = [np.full((J, 3), np.nan, f32) for _ in range(3)]
    for e, (n, S_, M) in enumerate(sums):
        assert n == 2 * n_close[e]
        if n:
            floats, _ = S.shape_row(n, S_, M)
            cen[e], spread[e], direction[e] = floats[0:3], floats[9:12], floats[15:18]
    sa, sb = shapes[uniq[:, 0]], shapes[uniq[:, 1]]
    na, nb, ca, cb, da, db = sa["normal"], sb["normal"], sa["centroid"], sb["centroid"], sa["plane_d"], sb["plane_d"]
    rows = np.zeros(J, P.REGION_JOINT_DTYPE)
    with np.errstate(all="ignore"):
        cos = dot3(na, nb)
        h_ab, h_ba = plane(na, cb, da), plane(nb, ca, db)
        e_a, e_b = plane(na, cen, da), plane(nb, cen, db)
        g, convex = normals_diff(na, ca, nb, cb)
        surface = n_close > 0
        coplanar = (cos >= cos_coplanar) & (np.abs(h_ab) <= plane_tol) & (np.abs(h_ba) <= plane_tol)
        kind = np.where(~surface, OCCLUSION, np.where(coplanar, COPLANAR, np.where((h_ab + h_ba).astype(f32) < 0, CONVEX, CONCAVE)))
    rows["a"], rows["b"], rows["n_pairs"], rows["n_close"] = uniq[:, 0], uniq[:, 1], n_pairs, n_close
    for name, val in (("centroid", cen), ("direction", direction), ("spread", spread), ("cos_angle", cos), ("delta_g", g), ("h_ab", h_ab), ("h_ba", h_ba), ("e_a", e_a), ("e_b", e_b)):
        rows[name] = canon(val).view(f32)
    rows["kind"] = kind.astype(u32) | np.where(convex, u32(REF_CONVEX), u32(0))
    return OK, rows, shapes, dict(n_regions=K, n_joints=J, n_surface=int(surface.sum()), reserved=0, n_pairs=int(n_pairs.sum()), n_close=int(n_close.sum()))


_refs = {}


def reference(P, key, sc, prm=None):
    """the reference of a scene, computed once per key and parameters and left unchanged"""
    prm = prm or (sc.get("depth_tol", DEFAULTS[0]),) + DEFAULTS[1:]
    k = (key, tuple(float(x) for x in prm))
    if k not in _refs:
        _refs[k] = ref_joints(P, sc["fmt"], sc["depth"], sc["labels"], sc["n_regions"], prm)
    return _refs[k]


def words_of(rows):
    return np.ascontiguousarray(rows).view(u32).reshape(len(rows), 20)


def assert_rows_equal(got, want, what=""):
    assert len(got) == len(want), "%s %d rows, want %d" % (what, len(got), len(want))
    g, w = words_of(got), words_of(want)
    if not np.array_equal(g, w):
        i, k = [int(a[0]) for a in np.nonzero(g != w)]
        raise AssertionError("%s row %d word %d: %#x, want %#x\ngot  %r\nwant %r" % (what, i, k, g[i, k], w[i, k], got[i], want[i]))


def params_of(P, prm):
    return P.JointParams(*[float(x) for x in prm])


def scene_params(sc):
    """(depth_tol, plane_tol, cos_coplanar) a scene runs with: its own depth_tol, the other defaults"""
    return (sc.get("depth_tol", DEFAULTS[0]),) + DEFAULTS[1:]


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------------------
def scene(P, which, width, height, depth_kind):
    return C.scene(P, which, width, height, depth_kind)


def analytic_scene(P, which, width=64, height=48):
    """f32 depths of exact planes: "ridge" two planes at +-30 degrees meeting on x = 0, nearest there; "valley" the same, farthest there; "one_plane" one tilted
    plane under both labels; "plate" a plate at 1 m in front of a wall at 2 m"""
    fmt = frame_format(P, width, height, "f32", "rgb8", 1.0)
    fmt.fx = fmt.fy = 60.0
    fmt.cx, fmt.cy = (width - 1) / 2.0, (height - 1) / 2.0
    uu, _ = np.meshgrid(np.arange(width, dtype=f64), np.arange(height, dtype=f64))
    rx = (uu - fmt.cx) / fmt.fx
    t = np.tan(np.radians(30.0))
    if which == "ridge":        # z = 1 + t |x|
        z = 1.0 / (1.0 - t * np.abs(rx))
    elif which == "valley":     # z = 1.5 - t |x|
        z = 1.5 / (1.0 + t * np.abs(rx))
    elif which == "one_plane":  # z = 1 + 0.3 x
        z = 1.0 / (1.0 - 0.3 * rx)
    elif which == "plate":
        z = np.where(uu < width / 2, 1.0, 2.0)
    else:
        raise ValueError(which)
    lab = (uu >= width / 2).astype(u32)
    return dict(fmt=fmt, depth=z.astype(f32), labels=lab, n_regions=2, depth_tol=0.05)


def own_region_scene(P, width, height):
    """every pixel its own region over a tilted plane: two rows a pixel, every border one close pair"""
    sc = analytic_scene(P, "one_plane", width, height)
    n = width * height
    return dict(sc, labels=np.arange(n, dtype=u32).reshape(height, width), n_regions=n)


def checker_scene(P, width, height):
    """own_region_scene with every seventh pixel invalid and a step in depth down the middle: surface borders, occlusions and labels over holes"""
    sc = own_region_scene(P, width, height)
    depth = sc["depth"].copy()
    depth[:, width // 2:] += f32(0.5)
    depth.reshape(-1)[3::7] = 0.0
    return dict(sc, depth=depth)


# ---- the device against the host function (tests/test_region_joints_gpu.py and its child processes) -----------------------------------------------------------
PREFILL = 0x5A5A5A5A
SMALL_FRAMES = [("blocks", 300, 7, "u16"), ("blocks", 257, 5, "f32"), ("blocks", 97, 61, "u16"), ("steps", 300, 7, "f32"), ("steps", 257, 5, "f32"), ("ridge", 64, 48, "f32"), ("valley", 64, 48, "f32"),
                ("one_plane", 64, 48, "f32"), ("plate", 64, 48, "f32"), ("own", 33, 31, "f32")]
_frames = {}


def small_frame(P, case):
    """a frame of SMALL_FRAMES, made once: blocks = the contacts' scene 1, steps = its scene 7 (close pairs, a in front and b in front on one border), the
    analytic scenes, own = every pixel its own region"""
    if case not in _frames:
        name, w, h, kind = case
        if name == "blocks":
            _frames[case] = scene(P, 1, w, h, kind)
        elif name == "steps":
            _frames[case] = scene(P, 7, w, h, kind)
        elif name == "own":
            _frames[case] = checker_scene(P, w, h)
        else:
            _frames[case] = analytic_scene(P, name, w, h)
    return _frames[case]


_host = {}


def host_joints(P, key, sc, prm=None):
    """(rows, shapes, result dict) of f3ds_region_joints_host on a scene, computed once per key and parameters and left unchanged"""
    prm = tuple(float(x) for x in (prm or scene_params(sc)))
    if (key, prm) not in _host:
        rows, shapes, res = P.region_joints_host(sc["depth"], sc["labels"], sc["n_regions"], sc["fmt"], params=params_of(P, prm), want_shapes=True)
        _host[(key, prm)] = (rows, shapes, res.as_dict())
    return _host[(key, prm)]


def gpu_joints(P, ctx, sc, prm=None, where="host", layout="tight", cap=64, count_only=False, want_shapes=True):
    """f3ds_region_joints on raw buffers: (rc, rows (all `cap` of them), n_out, shapes, result).  where "device": every buffer on the GPU.  Rows and shapes are
    prefilled with 0x5A5A5A5A words, n_out with 777, the result with sevens."""
    import ctypes
    f, dbuf, _ = buffers(sc["fmt"], sc["depth"], None, layout)
    lab = np.ascontiguousarray(sc["labels"], u32).reshape(-1)
    K = int(sc["n_regions"])
    p = params_of(P, prm or scene_params(sc))
    rows = np.full(20 * cap, PREFILL, u32)
    shapes = np.full(21 * K, PREFILL, u32)
    res = P.RegionJointsResult(7, 7, 7, 7, 7, 7)
    n_out = ctypes.c_size_t(777)
    if where == "device":
        import torch
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        dd, dl = dev(dbuf), dev(lab.view(np.int32))
        dr, ds = dev(np.full(max(20 * cap, 1), PREFILL, u32).view(np.int32)), dev(np.full(max(21 * K, 1), PREFILL, u32).view(np.int32))
        torch.cuda.synchronize()
        rc = ctx.lib.f3ds_region_joints(ctx.handle, ctypes.byref(f), ctypes.c_void_p(dd.data_ptr()), ctypes.c_void_p(dl.data_ptr()), K, ctypes.byref(p), 1,
                                        None if count_only else ctypes.c_void_p(dr.data_ptr()), cap, ctypes.c_void_p(ds.data_ptr()) if want_shapes and K else None, 1,
                                        ctypes.byref(n_out), ctypes.byref(res))
        torch.cuda.synchronize()
        rows = dr.cpu().numpy().view(u32)[:20 * cap].copy()
        shapes = ds.cpu().numpy().view(u32)[:21 * K].copy()
    else:
        rc = ctx.lib.f3ds_region_joints(ctx.handle, ctypes.byref(f), dbuf.ctypes.data, lab.ctypes.data, K, ctypes.byref(p), 0, None if count_only else rows.ctypes.data, cap,
                                        shapes.ctypes.data if want_shapes and K else None, 0, ctypes.byref(n_out), ctypes.byref(res))
    return rc, rows.view(P.REGION_JOINT_DTYPE), n_out.value, shapes.view(P.REGION_SHAPE_DTYPE), res


def check_device(P, ctx, sc, key, where="host", layout="tight", want_shapes=True, prm=None):
    """the device against the host function on one scene, bit for bit; returns the host function's (rows, result dict)"""
    wrows, wshapes, wres = host_joints(P, key, sc, prm)
    n = len(wrows)
    rc, rows, n_out, shapes, res = gpu_joints(P, ctx, sc, prm, where, layout, cap=n + 2, want_shapes=want_shapes)
    assert rc == 0 and n_out == n, (rc, n_out, n)
    assert_rows_equal(rows[:n], wrows, "%s %s" % (where, layout))
    assert (rows[n:].view(u32) == PREFILL).all()                                      # nothing behind the rows
    if want_shapes:
        S.assert_rows_equal(P, shapes, wshapes, "shapes %s" % where)
    else:
        assert (shapes.view(u32) == PREFILL).all()
    assert res.as_dict() == wres, (res.as_dict(), wres)
    return wrows, wres


def child_run(P, cap):
    """what a child process of the GPU test runs under its environment (F3DS_GRID_CAP = cap, or F3DS_RGJ_FIRST_CAP with cap 0): every small frame, host and
    device buffers, against the host function; returns {case: [rows, surface rows]} and asserts the launch width"""
    ctx = P.Context(0)
    out = {}
    try:
        for case in SMALL_FRAMES:
            sc = small_frame(P, case)
            for where in ("host", "device"):
                rows, res = check_device(P, ctx, sc, case, where, "padded" if where == "host" else "tight", want_shapes=where == "host")
            if cap:
                assert ctx.launch_shape() == (cap, cap, 1), ctx.launch_shape()
            out["%s-%dx%d" % case[:3]] = [len(rows), res["n_surface"]]
    finally:
        ctx.close()
    return out
