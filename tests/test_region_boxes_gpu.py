"""The region boxes on the device (f3ds_region_boxes: the shapes' three kernels, then d_box_frame, d_box_accum, d_box_finish in csrc/f3ds_boxes.inc) against
the reference of tests/region_boxes_common.py, bit for bit: the scenes and shapes of tests/test_region_boxes_cpu.py, host buffers and all-device buffers, at
the default launch width and at F3DS_GRID_CAP = 1 and 3.  At one workgroup the 5917 pixels of 97 x 61 are one span of 23 full trips and a ragged one, and
scene 3 (every pixel its own region) overflows the 128-slot LDS table many times over, so the minima and maxima go through the global path; at three the spans
end ragged and straddle rows.  What the device alone can get wrong: the second pass reading a frame the first has not finished, the per-lane frame gather
in a wave of several labels against the wave-uniform one, the two heads, the shape rows in each of their three places."""
import ctypes

import numpy as np
import pytest

import region_boxes_common as B
import region_shapes_common as S
import region_table_common as R
from region_table_common import NO
from rgbd_common import frame_images

pytestmark = pytest.mark.gpu
PREFILL = 0x5A5A5A5A
ALL_SCENES = R.SCENES + S.EXTRA
SEVENS = dict(n_regions=7, n_nonempty=7, n_labelled=7, n_clamped=7, n_inliers=7)
INF = float("inf")


def to_device(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
    torch.cuda.synchronize()
    return t


def gpu_boxes(P, ctx, fmt, depth, labels, n_regions, where="host", layout="tight", plane_tol=B.TOL, shapes="yes"):
    """f3ds_region_boxes on raw buffers: (rc, rows, shapes, result).  where "device": every buffer on the GPU.  shapes "no": a NULL pointer.  Rows and
    shapes are prefilled with 0x5A5A5A5A words."""
    f, dbuf, _ = R.buffers(fmt, depth, None, layout)
    lab = np.ascontiguousarray(labels, np.uint32).reshape(-1)
    K = int(n_regions)
    rows, srows = np.full(24 * K, PREFILL, np.uint32), np.full(21 * K, PREFILL, np.uint32)
    res = P.RegionBoxesResult(7, 7, 7, 7, 7)
    want = shapes == "yes" and K
    if where == "device":
        import torch
        dd, dl = to_device(dbuf), to_device(lab.view(np.int32))
        dr, ds = to_device(np.full(max(24 * K, 1), PREFILL, np.uint32).view(np.int32)), to_device(np.full(max(21 * K, 1), PREFILL, np.uint32).view(np.int32))
        rc = ctx.lib.f3ds_region_boxes(ctx.handle, ctypes.byref(f), ctypes.c_void_p(dd.data_ptr()), ctypes.c_void_p(dl.data_ptr()), K, float(plane_tol), 1,
                                       ctypes.c_void_p(dr.data_ptr()) if K else None, ctypes.c_void_p(ds.data_ptr()) if want else None, 1, ctypes.byref(res))
        torch.cuda.synchronize()
        rows = dr.cpu().numpy().view(np.uint32)[:24 * K].copy()
        srows = ds.cpu().numpy().view(np.uint32)[:21 * K].copy()
    else:
        rc = ctx.lib.f3ds_region_boxes(ctx.handle, ctypes.byref(f), dbuf.ctypes.data, lab.ctypes.data, K, float(plane_tol), 0, rows.ctypes.data if K else None,
                                       srows.ctypes.data if want else None, 0, ctypes.byref(res))
    return rc, rows.view(P.REGION_BOX_DTYPE), srows.view(P.REGION_SHAPE_DTYPE), res


def check(P, ctx, sc, key, where, layout, plane_tol=B.TOL, shapes="yes"):
    wrc, wrows, wshapes, wres = B.reference(P, key, sc, plane_tol)
    rc, rows, srows, res = gpu_boxes(P, ctx, sc["fmt"], sc["depth"], sc["labels"], sc["n_regions"], where, layout, plane_tol, shapes)
    assert rc == wrc == 0
    B.assert_rows_equal(P, rows, wrows, "%r %s %s" % (key, where, layout))
    if shapes == "yes":
        S.assert_rows_equal(P, srows, wshapes, "%r %s %s shapes" % (key, where, layout))
    else:
        assert (srows.view(np.uint32) == PREFILL).all()
    assert res.as_dict() == wres, (res.as_dict(), wres)
    return rows, wres


# ---- 1. the scenes, every shape, default and narrow launches ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [0, 1, 3])
@pytest.mark.parametrize("which", ALL_SCENES)
@pytest.mark.parametrize("width,height,depth_kind,layout", R.SHAPES)
def test_scene_equals_reference(P, gpu_ctx, monkeypatch, width, height, depth_kind, layout, which, cap):
    if cap:
        monkeypatch.setenv("F3DS_GRID_CAP", str(cap))
    sc = S.any_scene(P, which, width, height, depth_kind)
    for where in ("host", "device"):
        rows, res = check(P, gpu_ctx, sc, (which, width, height, depth_kind), where, layout)
    assert int(rows["n_pixels"].astype(np.int64).sum()) == res["n_labelled"] and int(rows["n_inliers"].astype(np.int64).sum()) == res["n_inliers"]
    if which == 3 and width * height > 128:
        assert res["n_nonempty"] > 10 * 128                                         # far more labels in a span than the LDS table has slots
    if which == 8:
        assert res["n_clamped"] > 0 or res["n_labelled"] == 0


@pytest.mark.parametrize("seed", R.RANDOM_SEEDS[:8])
def test_random_scene(P, gpu_ctx, monkeypatch, seed):
    if seed % 4 == 3:
        monkeypatch.setenv("F3DS_GRID_CAP", "1" if seed % 8 == 3 else "3")
    sc, _, layout = R.random_case(P, seed)
    check(P, gpu_ctx, sc, ("random", seed), "device" if seed % 3 == 1 else "host", layout)


@pytest.mark.parametrize("where", ["host", "device"])
def test_shapes_null_and_the_tolerances(P, gpu_ctx, where):
    """shapes NULL (the rows stay in scratch), a host pointer and a device pointer (check, above) give the same box rows; plane_tol 0 and +inf"""
    for width, height, depth_kind, layout in R.SHAPES[:2]:
        for which in (1, "thin"):
            sc = S.any_scene(P, which, width, height, depth_kind)
            key = (which, width, height, depth_kind)
            check(P, gpu_ctx, sc, key, where, layout, shapes="no")
            check(P, gpu_ctx, sc, key, where, layout, plane_tol=0.0)
            rows, res = check(P, gpu_ctx, sc, key, where, layout, plane_tol=INF, shapes="no")
            assert np.array_equal(rows["n_inliers"], rows["n_pixels"]) and res["n_inliers"] == res["n_labelled"]


def test_package_method_and_a_permutation(P, gpu_ctx):
    sc = R.scene(P, 1, 97, 61, "u16")
    K = sc["n_regions"]
    wrows, wshapes, wres = B.reference(P, (1, 97, 61, "u16"), sc)[1:]
    rows, res = gpu_ctx.region_boxes(sc["depth"], sc["labels"], K, sc["fmt"])
    B.assert_rows_equal(P, rows, wrows)
    assert res.as_dict() == wres and rows.dtype == P.REGION_BOX_DTYPE
    out, sout = np.zeros(K, P.REGION_BOX_DTYPE), np.zeros(K, P.REGION_SHAPE_DTYPE)
    got = gpu_ctx.region_boxes(sc["depth"], sc["labels"], K, sc["fmt"], plane_tol=B.TOL, rows_out=out, shapes_out=sout)
    assert got[0] is out and got[1] is sout and got[2].as_dict() == wres
    B.assert_rows_equal(P, out, wrows)
    S.assert_rows_equal(P, sout, wshapes)
    rows1, shapes1, _ = gpu_ctx.region_boxes(sc["depth"], sc["labels"], K, sc["fmt"], shapes_out=True)
    B.assert_rows_equal(P, rows1, wrows)
    S.assert_rows_equal(P, shapes1, wshapes)
    perm = np.random.default_rng(5).permutation(K).astype(np.uint32)
    lab = sc["labels"]
    moved = np.where(lab == NO, np.uint32(NO), perm[np.minimum(lab, K - 1)]).astype(np.uint32)
    rows2, res2 = gpu_ctx.region_boxes(sc["depth"], moved, K, sc["fmt"])
    B.assert_rows_equal(P, rows2[perm], rows)
    assert res2.as_dict() == res.as_dict()
    # device pointers through the package
    import torch
    dd, dl = to_device(sc["depth"].view(np.uint8)), to_device(lab.view(np.int32))
    dr, ds = torch.zeros(24 * K, dtype=torch.int32, device="cuda"), torch.zeros(21 * K, dtype=torch.int32, device="cuda")
    none, res3 = gpu_ctx.region_boxes(dd.data_ptr(), dl.data_ptr(), K, sc["fmt"], rows_out=dr.data_ptr(), on_device=True)
    torch.cuda.synchronize()
    assert none is None and res3.as_dict() == wres
    B.assert_rows_equal(P, dr.cpu().numpy().view(P.REGION_BOX_DTYPE), wrows)
    dr.zero_()
    got = gpu_ctx.region_boxes(dd.data_ptr(), dl.data_ptr(), K, sc["fmt"], rows_out=dr.data_ptr(), shapes_out=ds.data_ptr(), on_device=True)
    torch.cuda.synchronize()
    assert got[0] is None and got[1] is None and got[2].as_dict() == wres
    B.assert_rows_equal(P, dr.cpu().numpy().view(P.REGION_BOX_DTYPE), wrows)
    S.assert_rows_equal(P, ds.cpu().numpy().view(P.REGION_SHAPE_DTYPE), wshapes)


# ---- 2. errors, in both forms ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("where", ["host", "device"])
def test_a_bad_label_is_found_on_the_device_and_leaves_the_rows(P, gpu_ctx, monkeypatch, where, cap):
    if cap:
        monkeypatch.setenv("F3DS_GRID_CAP", str(cap))
    for width, height, depth_kind, layout in R.SHAPES:
        sc = R.scene(P, 1, width, height, depth_kind)
        K = sc["n_regions"]
        for at, value, invalid_depth in ((-1, K, False), (0, K + 5, False), (-1, 0xFFFFFFFE, True)):
            lab = sc["labels"].copy(); lab.reshape(-1)[at] = value
            depth = sc["depth"].copy()
            if invalid_depth:
                depth.reshape(-1)[at] = 0
            rc, rows, srows, res = gpu_boxes(P, gpu_ctx, sc["fmt"], depth, lab, K, where, layout)
            assert rc == P.ERR_ARG
            assert (rows.view(np.uint32) == PREFILL).all() and (srows.view(np.uint32) == PREFILL).all() and res.as_dict() == SEVENS
        # and the context still answers
        check(P, gpu_ctx, sc, (1, width, height, depth_kind), where, layout)


def test_argument_errors(P, gpu_ctx):
    lib = gpu_ctx.lib
    sc = R.scene(P, 1, 3, 2, "u16")
    fmt, K = R.with_color(P, sc["fmt"], "rgb8"), sc["n_regions"]
    d, l = sc["depth"], sc["labels"]
    rows, shapes = np.zeros(K, P.REGION_BOX_DTYPE), np.zeros(K, P.REGION_SHAPE_DTYPE)
    for on_dev in (0, 1):      # (every one of these is refused before a buffer is looked at: host pointers do for both forms)
        good = [gpu_ctx.handle, ctypes.byref(fmt), d.ctypes.data, l.ctypes.data, K, 0.01, on_dev, rows.ctypes.data, shapes.ctypes.data, on_dev, None]
        for k in (0, 1, 2, 3, 7):
            a = list(good); a[k] = None
            assert lib.f3ds_region_boxes(*a) == P.ERR_ARG, k
        for fields in (dict(width=0), dict(depth_type=7), dict(fx=0.0), dict(fy=float("nan")), dict(depth_scale=0.0), dict(cx=float("inf")), dict(depth_pitch=3)):
            f = fmt.copy()
            for k, v in fields.items():
                setattr(f, k, v)
            a = list(good); a[1] = ctypes.byref(f)
            assert lib.f3ds_region_boxes(*a) == P.ERR_ARG, fields
        for tol in (-0.5, -INF, float("nan")):
            a = list(good); a[5] = tol
            assert lib.f3ds_region_boxes(*a) == P.ERR_ARG, tol
        a = list(good); a[4] = 0x01000000
        assert lib.f3ds_region_boxes(*a) == P.ERR_UNSUPPORTED
        a[5] = -1.0
        assert lib.f3ds_region_boxes(*a) == P.ERR_ARG                               # a bad tolerance comes before too many regions
    # the colour fields are not looked at; n_regions == 0; a frame without a labelled pixel
    f = fmt.copy(); f.color_format = 99; f.color_pitch = 1
    res = P.RegionBoxesResult()
    assert lib.f3ds_region_boxes(gpu_ctx.handle, ctypes.byref(f), d.ctypes.data, l.ctypes.data, K, 0.01, 0, rows.ctypes.data, shapes.ctypes.data, 0, ctypes.byref(res)) == 0
    wrows, wshapes = B.ref_boxes(P, fmt, d, l, K)[1:3]
    B.assert_rows_equal(P, rows, wrows)
    S.assert_rows_equal(P, shapes, wshapes)
    none = np.full((2, 3), NO, np.uint32)
    assert lib.f3ds_region_boxes(gpu_ctx.handle, ctypes.byref(fmt), d.ctypes.data, none.ctypes.data, 0, 0.01, 0, None, None, 0, ctypes.byref(res)) == 0
    assert res.as_dict() == dict(n_regions=0, n_nonempty=0, n_labelled=0, n_clamped=0, n_inliers=0)
    assert lib.f3ds_region_boxes(gpu_ctx.handle, ctypes.byref(fmt), d.ctypes.data, l.ctypes.data, 0, 0.01, 0, None, None, 0, None) == P.ERR_ARG      # label 0 >= 0 regions
    rc, rows, srows, res = gpu_boxes(P, gpu_ctx, fmt, np.zeros((2, 3), np.uint16), l, K)
    assert rc == 0 and res.as_dict() == dict(n_regions=K, n_nonempty=0, n_labelled=0, n_clamped=0, n_inliers=0)
    assert (B.words_of(rows) == B.EMPTY_ROW).all() and (S.words_of(srows) == np.array([0] + [R.QNAN] * 20, np.uint32)).all()


# ---- 3. end to end -----------------------------------------------------------------------------------------------------------------------------------------

def same(a, b):
    """two answers of a context (a tuple or a dict of arrays), byte for byte"""
    if isinstance(a, dict):
        a, b = [a[k] for k in sorted(a)], [b[k] for k in sorted(a)]
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_the_boxes_of_a_segmented_frame_and_the_context_afterwards(P):
    fmt, depth, color = frame_images(P, 7, 160, 120)
    prm = P.launch_params(voxel_res=0.02, seed_res=0.2)
    ctx, other = P.Context(0), P.Context(0)
    try:
        lab = ctx.segment_rgbd(depth, color, fmt, prm); K = int(ctx.result.n_regions)
        assert np.array_equal(other.segment_rgbd(depth, color, fmt, prm), lab) and K > 10
        rows, shapes, res = ctx.region_boxes(depth, lab, K, fmt, shapes_out=True)
        wrc, wrows, wshapes, wres = B.ref_boxes(P, fmt, depth, lab, K)
        assert wrc == 0 and res.as_dict() == wres
        B.assert_rows_equal(P, rows, wrows)
        S.assert_rows_equal(P, shapes, wshapes)
        assert int(rows["n_pixels"].astype(np.int64).sum()) == int((lab != NO).sum()) == res.n_labelled and 0 < res.n_nonempty <= K
        assert B.assert_contained(rows, shapes, fmt, depth, lab) == res.n_labelled
        # the context answers as one that never made the call
        assert same(ctx.regions(), other.regions()) and same(ctx.voxel_cloud(), other.voxel_cloud())
        assert np.array_equal(ctx.recluster(prm), other.recluster(prm)) and ctx.result.n_regions == other.result.n_regions
        # one lower level of the same run
        levels, nreg = ctx.labels_at_thresholds([0.1])
        K1 = int(nreg[0])
        assert K1 >= K
        rows1, res1 = ctx.region_boxes(depth, levels[0], K1, fmt)
        wrows1, _, wres1 = B.ref_boxes(P, fmt, depth, levels[0], K1)[1:]
        B.assert_rows_equal(P, rows1, wrows1)
        assert res1.as_dict() == wres1 and res1.n_labelled == res.n_labelled
        assert same(ctx.regions(), other.regions())
    finally:
        ctx.close(); other.close()


def test_the_shapes_and_the_table_around_the_boxes_on_one_context(P, gpu_ctx):
    """region_shapes and region_table before and after region_boxes on one context: identical rows (pass one of the boxes adds into the shapes' accumulators)"""
    sc = R.scene(P, 1, 97, 61, "u16")
    K = sc["n_regions"]
    s0, sr0 = gpu_ctx.region_shapes(sc["depth"], sc["labels"], K, sc["fmt"])
    t0, tr0 = gpu_ctx.region_table(sc["depth"], sc["labels"], K, sc["fmt"])
    rows, shapes, res = gpu_ctx.region_boxes(sc["depth"], sc["labels"], K, sc["fmt"], shapes_out=True)
    s1, sr1 = gpu_ctx.region_shapes(sc["depth"], sc["labels"], K, sc["fmt"])
    t1, tr1 = gpu_ctx.region_table(sc["depth"], sc["labels"], K, sc["fmt"])
    S.assert_rows_equal(P, s1, s0)
    S.assert_rows_equal(P, shapes, s0)
    R.assert_rows_equal(P, t1, t0)
    assert sr0.as_dict() == sr1.as_dict() and tr0.as_dict() == tr1.as_dict() and {k: res.as_dict()[k] for k in S.RESULT_FIELDS} == sr0.as_dict()
    B.assert_rows_equal(P, gpu_ctx.region_boxes(sc["depth"], sc["labels"], K, sc["fmt"])[0], rows)      # and the boxes again
