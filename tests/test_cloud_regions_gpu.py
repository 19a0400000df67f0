"""The region rows of a point cloud on the device (f3ds_cloud_regions: d_cloud_init, [d_cloud_keys, the radix sort,] d_cloud_accum, d_cloud_finish and, with boxes,
d_box_frame, d_cloud_box_accum, d_box_finish in csrc/f3ds_cloud.inc) against the host function f3ds_cloud_regions_host, word for word -- the host function
itself is pinned to the family and to a reference of its own in tests/test_cloud_regions_cpu.py.

Every cloud runs with host buffers and with all-device buffers, with and without boxes, on the direct and on the ordered walk (the development switch
F3DS_CLOUD_PATH) and at the default launch width and F3DS_GRID_CAP = 1 and 3: the bits are the same in all, and F3DS_DBG_CLOUD_PATH reports the walk.  The
clouds: every image scene of the CPU test as a cloud, on its four shapes (scene 3 a region per point), the clouds of cloud_regions_common.CLOUDS (K = 3000 scattered: forced
onto the direct walk every trip of a workgroup overflows the 128-slot table; on the ordered walk the table is flushed and cleared trip after trip), and sizes
that straddle the launch (63, 64, 65 points; 257, one more than a workgroup; 769, one more than a span each for three workgroups).  Then: the labels of
f3ds_segment and of the lowest level of f3ds_labels_at_thresholds on the golden PCD, device-resident; points16 == NULL after f3ds_segment_rgbd; the context
untouched; the errors."""
import ctypes

import numpy as np
import pytest

import cloud_regions_common as C
import region_boxes_common as B
import region_shapes_common as S
import region_table_common as R
from conftest import ALL_DEBUG, FIXTURE_PCD
from region_table_common import NO
from rgbd_common import frame_images

pytestmark = pytest.mark.gpu
PREFILL = 0x5A5A5A5A
SEVENS = dict(n_regions=7, n_nonempty=7, n_labelled=7, n_clamped=7, n_inliers=7)
PATHS = ["direct", "ordered"]
CAPS = [0, 1, 3]
SIZES = ["n%d" % n for n in C.LAUNCH_SIZES]
ALL_SCENES = R.SCENES + S.EXTRA


def to_device(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
    torch.cuda.synchronize()
    return t


def gpu_cloud(P, ctx, pts, labels, n_regions, where="host", tol=C.TOL, fold=0, boxes="yes", null_points=False):
    """f3ds_cloud_regions on raw buffers: (rc, rows, boxes, result).  where "device": every buffer on the GPU.  boxes "no": a NULL pointer.  Rows and boxes are
    prefilled with 0x5A5A5A5A words, the result with sevens.  null_points: points16 == NULL (the context's own records)."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    lab = np.ascontiguousarray(labels, np.uint32).reshape(-1)
    n, K = len(lab), int(n_regions)
    rows, brows = np.full(32 * K, PREFILL, np.uint32), np.full(24 * K, PREFILL, np.uint32)
    res = P.CloudRegionsResult(7, 7, 7, 7, 7)
    prm = C.params_of(P, tol, fold)
    want = boxes == "yes"
    spare = np.zeros(24, np.float32)
    vp = ctypes.c_void_p
    if where == "device":
        import torch
        dp, dl = to_device(pts if n else spare.reshape(-1, 4)[:1]), to_device((lab if n else np.zeros(1, np.uint32)).view(np.int32))
        dr, db = to_device(np.full(max(32 * K, 1), PREFILL, np.uint32).view(np.int32)), to_device(np.full(max(24 * K, 1), PREFILL, np.uint32).view(np.int32))
        rc = ctx.lib.f3ds_cloud_regions(ctx.handle, None if null_points else vp(dp.data_ptr()), n, vp(dl.data_ptr()), K, ctypes.byref(prm), 1, vp(dr.data_ptr()) if K else None,
                                        vp(db.data_ptr()) if want else None, 1, ctypes.byref(res))
        torch.cuda.synchronize()
        rows = dr.cpu().numpy().view(np.uint32)[:32 * K].copy()
        brows = db.cpu().numpy().view(np.uint32)[:24 * K].copy()
    else:
        rc = ctx.lib.f3ds_cloud_regions(ctx.handle, None if null_points else (pts.ctypes.data if n else spare.ctypes.data), n, lab.ctypes.data if n else spare.ctypes.data, K,
                                        ctypes.byref(prm), 0, rows.ctypes.data if K else None, (brows.ctypes.data if K else spare.ctypes.data) if want else None, 0, ctypes.byref(res))
    return rc, rows.view(P.CLOUD_REGION_DTYPE), brows.view(P.REGION_BOX_DTYPE), res


_host = {}


def host_rows(P, key, pts, labels, K, tol=C.TOL, fold=0):
    """what the host function says of a cloud, computed once per key and left unchanged: (rows, boxes, result dict)"""
    if key not in _host:
        rc, rows, boxes, res = C.c_cloud(P, pts, labels, K, tol, fold)
        assert rc == 0
        _host[key] = (rows, boxes, res.as_dict())
    return _host[key]


def check(P, ctx, key, pts, labels, K, where, boxes="yes", tol=C.TOL, fold=0, path=None):
    wrows, wboxes, wres = host_rows(P, key, pts, labels, K, tol, fold)
    rc, rows, brows, res = gpu_cloud(P, ctx, pts, labels, K, where, tol, fold, boxes)
    what = "%r %s boxes %s path %s" % (key, where, boxes, path)
    assert rc == 0, what
    C.assert_rows_equal(rows, wrows, what)
    if boxes == "yes":
        B.assert_rows_equal(P, brows, wboxes, what)
        assert res.as_dict() == wres, (what, res.as_dict(), wres)
    else:
        assert (brows.view(np.uint32) == PREFILL).all() and res.as_dict() == dict(wres, n_inliers=0), what
    if path:
        assert ctx.cloud_path() == path, what
    return rows, res


def switches(monkeypatch, path, cap):
    if path:
        monkeypatch.setenv("F3DS_CLOUD_PATH", path)
    else:
        monkeypatch.delenv("F3DS_CLOUD_PATH", raising=False)
    if cap:
        monkeypatch.setenv("F3DS_GRID_CAP", str(cap))
    else:
        monkeypatch.delenv("F3DS_GRID_CAP", raising=False)


# ---- 1. every cloud, both walks, default and narrow launches ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", C.CLOUDS + SIZES)
def test_cloud_equals_the_host_function(P, gpu_ctx, monkeypatch, name, path, cap):
    switches(monkeypatch, path, cap)
    c = C.cloud(name)
    for where in ("host", "device"):
        for boxes in ("yes", "no"):
            check(P, gpu_ctx, name, c["pts"], c["labels"], c["K"], where, boxes, c["tol"], c["fold"], path)
    if cap:
        assert gpu_ctx.launch_shape()[:2] == (cap, cap)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("which", ALL_SCENES)
@pytest.mark.parametrize("width,height,depth_kind,layout", R.SHAPES)
def test_image_scene_as_a_cloud(P, gpu_ctx, monkeypatch, width, height, depth_kind, layout, which, path, cap):
    """every scene and shape of tests/test_cloud_regions_cpu.py, item 1 (the records of f3ds_deproject under the scene's labels), host and device buffers, with
    and without boxes; `layout` is the images' and does not reach the records"""
    switches(monkeypatch, path, cap)
    key = (which, width, height, depth_kind)
    sc, pts = C.scene_cloud(P, *key)
    for where in ("host", "device"):
        for boxes in ("yes", "no"):
            rows, res = check(P, gpu_ctx, ("scene",) + key, pts, sc["labels"], sc["n_regions"], where, boxes, path=path)
    assert int(rows["n_points"].astype(np.int64).sum()) == res.n_labelled
    if which == 3 and width * height > 128:
        assert res.n_nonempty > 10 * 128                                            # far more labels than the LDS table has slots
    if which == 8:
        assert res.n_clamped > 0 or res.n_labelled == 0


def test_the_documented_choice_without_a_switch(P, gpu_ctx, monkeypatch):
    """K = 23 takes the direct walk, K = 3000 scattered the ordered one; the threshold itself, K = 96 against 97, with the same points"""
    switches(monkeypatch, None, 0)
    for name, want in (("K23", "direct"), ("K3000", "ordered"), ("empty", "direct"), ("K200", "ordered")):
        c = C.cloud(name)
        check(P, gpu_ctx, name, c["pts"], c["labels"], c["K"], "host", path=want)
    c = C.cloud("K23")
    for K, want in ((96, "direct"), (97, "ordered")):
        check(P, gpu_ctx, ("K23", K), c["pts"], c["labels"], K, "device", path=want)


def test_package_method(P, gpu_ctx, monkeypatch):
    switches(monkeypatch, None, 0)
    c = C.cloud("K200")
    wrows, wboxes, wres = host_rows(P, "K200", c["pts"], c["labels"], c["K"])
    rows, res = gpu_ctx.cloud_regions(c["pts"], c["labels"], c["K"])
    C.assert_rows_equal(rows, wrows)
    assert res.as_dict() == dict(wres, n_inliers=0) and rows.dtype == P.CLOUD_REGION_DTYPE
    out, bout = np.zeros(c["K"], P.CLOUD_REGION_DTYPE), np.zeros(c["K"], P.REGION_BOX_DTYPE)
    got = gpu_ctx.cloud_regions(c["pts"], c["labels"], c["K"], params=P.default_cloud_params(), rows_out=out, boxes_out=bout)
    assert got[0] is out and got[1] is bout and got[2].as_dict() == wres
    C.assert_rows_equal(out, wrows); B.assert_rows_equal(P, bout, wboxes)
    rows1, boxes1, _ = gpu_ctx.cloud_regions(c["pts"], c["labels"], c["K"], boxes_out=True)
    C.assert_rows_equal(rows1, wrows); B.assert_rows_equal(P, boxes1, wboxes)
    import torch
    dp, dl = to_device(c["pts"]), to_device(c["labels"].view(np.int32))
    dr, db = torch.zeros(32 * c["K"], dtype=torch.int32, device="cuda"), torch.zeros(24 * c["K"], dtype=torch.int32, device="cuda")
    got = gpu_ctx.cloud_regions(dp, dl, c["K"], rows_out=dr, boxes_out=db, n=len(c["labels"]), on_device=True)
    torch.cuda.synchronize()
    assert got[0] is None and got[1] is None and got[2].as_dict() == wres
    C.assert_rows_equal(dr.cpu().numpy().view(P.CLOUD_REGION_DTYPE), wrows); B.assert_rows_equal(P, db.cpu().numpy().view(P.REGION_BOX_DTYPE), wboxes)
    rows0, res0 = gpu_ctx.cloud_regions(np.zeros((0, 4), np.float32), np.zeros(0, np.uint32), 2)
    assert (C.words_of(rows0) == C.EMPTY_ROW).all() and res0.n_labelled == 0


# ---- 2. errors -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("where", ["host", "device"])
def test_a_bad_label_is_found_on_the_device_and_leaves_the_rows(P, gpu_ctx, monkeypatch, where, path):
    switches(monkeypatch, path, 0)
    for name in ("n65", "K200"):
        c = C.cloud(name)
        for at, value, not_finite in ((-1, c["K"], False), (0, c["K"] + 5, False), (7, 0xFFFFFFFE, True)):
            lab, pts = c["labels"].copy(), c["pts"].copy()
            lab[at] = value
            if not_finite:
                pts[at, 1] = np.nan      # the bad label sits on a point that is not finite, and nowhere else
            for boxes in ("yes", "no"):
                rc, rows, brows, res = gpu_cloud(P, gpu_ctx, pts, lab, c["K"], where, boxes=boxes)
                assert rc == P.ERR_ARG
                assert (rows.view(np.uint32) == PREFILL).all() and (brows.view(np.uint32) == PREFILL).all() and res.as_dict() == SEVENS
        check(P, gpu_ctx, name, c["pts"], c["labels"], c["K"], where, path=path)      # and the context still answers


def test_argument_errors_in_order(P, gpu_ctx):
    lib = gpu_ctx.lib
    c = C.cloud("n65")
    pts, lab, K = c["pts"], c["labels"], c["K"]
    rows = np.frombuffer(b"\xA5" * (128 * K), P.CLOUD_REGION_DTYPE).copy()
    boxes = np.frombuffer(b"\xA5" * (96 * K), P.REGION_BOX_DTYPE).copy()
    res = P.CloudRegionsResult(7, 7, 7, 7, 7)
    ok, neg, nan = P.CloudParams(0.01, 0), P.CloudParams(-0.5, 0), P.CloudParams(float("nan"), 0)

    def untouched():
        return (rows.view(np.uint8) == 0xA5).all() and (boxes.view(np.uint8) == 0xA5).all() and res.as_dict() == SEVENS
    for on_dev in (0, 1):      # (every one of these is refused before a buffer is looked at: host pointers do for both forms)
        good = [gpu_ctx.handle, pts.ctypes.data, len(lab), lab.ctypes.data, K, ctypes.byref(ok), on_dev, rows.ctypes.data, boxes.ctypes.data, on_dev, ctypes.byref(res)]

        def with_(**kw):
            a = list(good)
            for k, v in kw.items():
                a[dict(ctx=0, pts=1, n=2, lab=3, K=4, prm=5, rows=7)[k]] = v
            return a
        for a in (with_(ctx=None), with_(lab=None), with_(rows=None), with_(prm=ctypes.byref(neg)), with_(prm=ctypes.byref(nan)), with_(prm=ctypes.byref(neg), K=0x01000000),
                  with_(lab=None, n=0x80000000)):
            assert lib.f3ds_cloud_regions(*a) == P.ERR_ARG and untouched()
        assert lib.f3ds_cloud_regions(*with_(K=0x01000000)) == P.ERR_UNSUPPORTED and untouched()
        assert lib.f3ds_cloud_regions(*with_(n=0x80000000)) == P.ERR_UNSUPPORTED and untouched()
    # NULL params are the defaults; n_regions == 0 under no labels; any label then is out of range
    assert lib.f3ds_cloud_regions(gpu_ctx.handle, pts.ctypes.data, len(lab), lab.ctypes.data, K, None, 0, rows.ctypes.data, boxes.ctypes.data, 0, ctypes.byref(res)) == 0
    wrows, wboxes, wres = host_rows(P, "n65", pts, lab, K)
    C.assert_rows_equal(rows, wrows); B.assert_rows_equal(P, boxes, wboxes); assert res.as_dict() == wres
    none = np.full(len(lab), NO, np.uint32)
    assert lib.f3ds_cloud_regions(gpu_ctx.handle, pts.ctypes.data, len(lab), none.ctypes.data, 0, None, 0, None, None, 0, ctypes.byref(res)) == 0
    assert res.as_dict() == dict(n_regions=0, n_nonempty=0, n_labelled=0, n_clamped=0, n_inliers=0)
    assert lib.f3ds_cloud_regions(gpu_ctx.handle, pts.ctypes.data, len(lab), lab.ctypes.data, 0, None, 0, None, None, 0, None) == P.ERR_ARG


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------------------------------------
def same(a, b):
    """two answers of a context (a tuple or a dict of arrays), byte for byte"""
    if isinstance(a, dict):
        a, b = [a[k] for k in sorted(a)], [b[k] for k in sorted(a)]
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_the_regions_of_a_segmented_cloud_on_device_resident_labels(P, monkeypatch):
    """f3ds_segment on the golden PCD with the points and the labels on the device: the rows of the device labels equal the host function on the downloaded
    ones, and so for the lowest level of f3ds_labels_at_thresholds, the one with the most regions.  The context's points are the caller's: points16 == NULL is
    a logic error there."""
    import torch
    switches(monkeypatch, None, 0)
    pts = P.read_pcd(FIXTURE_PCD)
    n = len(pts)
    prm = P.launch_params()
    ctx = P.Context(0)
    try:
        dp = to_device(pts)
        dl = torch.zeros(n, dtype=torch.int32, device="cuda")
        ctx.segment(dp.data_ptr(), prm, labels_out=dl.data_ptr(), n=n, on_device=True)
        K = int(ctx.result.n_regions)
        levels = torch.zeros(n, dtype=torch.int32, device="cuda")
        _, nreg = ctx.labels_at_thresholds([0.0], out=levels, on_device=True)
        K0 = int(nreg[0])
        assert K0 >= K > 1
        finite = np.isfinite(pts[:, :3]).all(axis=1)
        for d_lab, k, fold in ((dl, K, 0), (levels, K0, 0), (levels, K0, 1)):
            lab = d_lab.cpu().numpy().view(np.uint32)
            rc, wrows, wboxes, wres = C.c_cloud(P, pts, lab, k, fold=fold)
            assert rc == 0
            dr, db = torch.zeros(32 * k, dtype=torch.int32, device="cuda"), torch.zeros(24 * k, dtype=torch.int32, device="cuda")
            _, _, res = ctx.cloud_regions(dp, d_lab, k, params=C.params_of(P, fold=fold), rows_out=dr, boxes_out=db, n=n, on_device=True)
            torch.cuda.synchronize()
            rows = dr.cpu().numpy().view(P.CLOUD_REGION_DTYPE)
            C.assert_rows_equal(rows, wrows); B.assert_rows_equal(P, db.cpu().numpy().view(P.REGION_BOX_DTYPE), wboxes)
            assert res.as_dict() == wres.as_dict()
            assert int(rows["n_points"].astype(np.int64).sum()) == int(((lab != NO) & finite).sum()) == res.n_labelled
            assert ctx.cloud_path() == P_path(k)
        lab = dl.cpu().numpy().view(np.uint32)
        rows = np.zeros(K, P.CLOUD_REGION_DTYPE); res = P.CloudRegionsResult(7, 7, 7, 7, 7)
        assert ctx.lib.f3ds_cloud_regions(ctx.handle, None, n, lab.ctypes.data, K, None, 0, rows.ctypes.data, None, 0, ctypes.byref(res)) == C.ERR_LOGIC
        assert res.as_dict() == SEVENS and not rows.view(np.uint8).any()
    finally:
        ctx.close()


def P_path(K):
    return "direct" if K <= 96 else "ordered"


def test_null_points_after_segment_rgbd_and_the_context_afterwards(P, monkeypatch):
    """points16 == NULL gives the bits of passing f3ds_get_points' records; with another count it is an argument error; recluster and every F3DS_DBG_* array
    are the same before and after the cloud calls"""
    switches(monkeypatch, None, 0)
    fmt, depth, color = frame_images(P, 7, 160, 120)
    prm = P.launch_params(voxel_res=0.02, seed_res=0.2)
    ctx, other = P.Context(0), P.Context(0)
    try:
        assert ctx.cloud_path() is None
        lab = ctx.segment_rgbd(depth, color, fmt, prm); K = int(ctx.result.n_regions)
        assert np.array_equal(other.segment_rgbd(depth, color, fmt, prm), lab) and K > 10
        before = {name: ctx.debug(name) for name in ALL_DEBUG}
        pts = ctx.points()
        assert np.array_equal(pts.view(np.uint32), P.deproject(fmt, depth, color).view(np.uint32))
        rc, wrows, wboxes, wres = C.c_cloud(P, pts, lab, K)
        assert rc == 0
        for path in (None, "direct", "ordered"):
            switches(monkeypatch, path, 0)
            for where in ("host", "device"):
                rc, rows, boxes, res = gpu_cloud(P, ctx, pts, lab, K, where, null_points=True)
                assert rc == 0 and res.as_dict() == wres.as_dict()
                C.assert_rows_equal(rows, wrows); B.assert_rows_equal(P, boxes, wboxes)
                rc, rows, boxes, res = gpu_cloud(P, ctx, pts, lab, K, where)
                assert rc == 0 and res.as_dict() == wres.as_dict()
                C.assert_rows_equal(rows, wrows); B.assert_rows_equal(P, boxes, wboxes)
        switches(monkeypatch, None, 0)
        rows, res = ctx.cloud_regions(None, lab, K)
        C.assert_rows_equal(rows, wrows)
        rc, rows, boxes, res = gpu_cloud(P, ctx, pts[:-1], lab[:-1], K, "host", null_points=True)      # another count than the context's records
        assert rc == P.ERR_ARG and (rows.view(np.uint32) == PREFILL).all() and res.as_dict() == SEVENS
        # the image family on the same frame says the same: the table's and the shapes' words
        trows, _ = ctx.region_table(depth, lab, K, fmt, color=color)
        w, tw = C.words_of(wrows), R.words_of(trows)
        assert np.array_equal(w[:, :2], tw[:, :2]) and np.array_equal(w[:, 2:14], tw[:, 6:18])
        srows, _ = ctx.region_shapes(depth, lab, K, fmt)
        assert np.array_equal(w[:, 14:31], S.words_of(srows)[:, 4:21])
        # the context answers as one that never made the calls
        after = {name: ctx.debug(name) for name in ALL_DEBUG}
        assert same(before, after)
        assert same(ctx.regions(), other.regions()) and same(ctx.voxel_cloud(), other.voxel_cloud())
        assert np.array_equal(ctx.recluster(prm), other.recluster(prm)) and ctx.result.n_regions == other.result.n_regions
        assert np.array_equal(ctx.points().view(np.uint32), pts.view(np.uint32))
    finally:
        ctx.close(); other.close()
