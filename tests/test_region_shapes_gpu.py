"""The region shapes on the device (f3ds_region_shapes: d_shape_init, d_shape_accum, d_shape_finish in csrc/f3ds_shapes.inc) against the reference of
tests/region_shapes_common.py, bit for bit: the scenes and shapes of tests/test_region_shapes_cpu.py, host buffers and all-device buffers, at the default
launch width and at F3DS_GRID_CAP = 1 and 3.  At one workgroup the 5917 pixels of 97 x 61 are one span of 23 full trips and a ragged one, and scene 3 (every
pixel its own region) overflows the 128-slot LDS table many times over; at three the spans end ragged and straddle rows.  What the device alone can get
wrong: the 128-bit integer to f64 conversion, the f64 divisions and square roots of the finish, the half-sums."""
import ctypes

import numpy as np
import pytest

import region_shapes_common as S
import region_table_common as R
from region_table_common import NO
from rgbd_common import frame_images

pytestmark = pytest.mark.gpu
PREFILL = 0x5A5A5A5A
ALL_SCENES = R.SCENES + S.EXTRA


def to_device(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
    torch.cuda.synchronize()
    return t


def gpu_shapes(P, ctx, fmt, depth, labels, n_regions, where="host", layout="tight"):
    """f3ds_region_shapes on raw buffers: (rc, rows, result).  where "device": every buffer on the GPU.  The rows are prefilled with 0x5A5A5A5A words."""
    f, dbuf, _ = R.buffers(fmt, depth, None, layout)
    lab = np.ascontiguousarray(labels, np.uint32).reshape(-1)
    K = int(n_regions)
    rows = np.full(21 * K, PREFILL, np.uint32)
    res = P.RegionShapesResult(7, 7, 7, 7)
    if where == "device":
        import torch
        dd, dl, dr = to_device(dbuf), to_device(lab.view(np.int32)), to_device(np.full(max(21 * K, 1), PREFILL, np.uint32).view(np.int32))
        rc = ctx.lib.f3ds_region_shapes(ctx.handle, ctypes.byref(f), ctypes.c_void_p(dd.data_ptr()), ctypes.c_void_p(dl.data_ptr()), K, 1,
                                        ctypes.c_void_p(dr.data_ptr()) if K else None, 1, ctypes.byref(res))
        torch.cuda.synchronize()
        rows = dr.cpu().numpy().view(np.uint32)[:21 * K].copy()
    else:
        rc = ctx.lib.f3ds_region_shapes(ctx.handle, ctypes.byref(f), dbuf.ctypes.data, lab.ctypes.data, K, 0, rows.ctypes.data if K else None, 0, ctypes.byref(res))
    return rc, rows.view(P.REGION_SHAPE_DTYPE), res


def check(P, ctx, sc, key, where, layout):
    wrc, wrows, wres, _ = S.reference(P, key, sc)
    rc, rows, res = gpu_shapes(P, ctx, sc["fmt"], sc["depth"], sc["labels"], sc["n_regions"], where, layout)
    assert rc == wrc == 0
    S.assert_rows_equal(P, rows, wrows, "%r %s %s" % (key, where, layout))
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
    assert int(rows["n_pixels"].astype(np.int64).sum()) == res["n_labelled"]
    if which == 3 and width * height > 128:
        assert res["n_nonempty"] > 10 * 128                                         # far more labels in a span than the LDS table has slots
    if which in (8, "8+2"):
        assert res["n_clamped"] > 0 or res["n_labelled"] == 0
    if which == "8+2" and width * height > 6:
        assert S.reference(P, (which, width, height, depth_kind), sc)[3][0][2][5] > 2 ** 64      # M_zz: sums kept in 64 bits cannot pass


@pytest.mark.parametrize("seed", R.RANDOM_SEEDS[:8])
def test_random_scene(P, gpu_ctx, monkeypatch, seed):
    if seed % 4 == 3:
        monkeypatch.setenv("F3DS_GRID_CAP", "1" if seed % 8 == 3 else "3")
    sc, _, layout = R.random_case(P, seed)
    check(P, gpu_ctx, sc, ("random", seed), "device" if seed % 3 == 1 else "host", layout)


def test_package_method_and_a_permutation(P, gpu_ctx):
    sc = R.scene(P, 1, 97, 61, "u16")
    K = sc["n_regions"]
    rows, res = gpu_ctx.region_shapes(sc["depth"], sc["labels"], K, sc["fmt"])
    wrows, wres = S.reference(P, (1, 97, 61, "u16"), sc)[1:3]
    S.assert_rows_equal(P, rows, wrows)
    assert res.as_dict() == wres and rows.dtype == P.REGION_SHAPE_DTYPE
    out = np.zeros(K, P.REGION_SHAPE_DTYPE)
    assert gpu_ctx.region_shapes(sc["depth"], sc["labels"], K, sc["fmt"], rows_out=out)[0] is out
    S.assert_rows_equal(P, out, wrows)
    perm = np.random.default_rng(5).permutation(K).astype(np.uint32)
    lab = sc["labels"]
    moved = np.where(lab == NO, np.uint32(NO), perm[np.minimum(lab, K - 1)]).astype(np.uint32)
    rows2, res2 = gpu_ctx.region_shapes(sc["depth"], moved, K, sc["fmt"])
    S.assert_rows_equal(P, rows2[perm], rows)
    assert res2.as_dict() == res.as_dict()
    # device pointers through the package
    import torch
    dd, dl = to_device(sc["depth"].view(np.uint8)), to_device(lab.view(np.int32))
    dr = torch.zeros(21 * K, dtype=torch.int32, device="cuda")
    none, res3 = gpu_ctx.region_shapes(dd.data_ptr(), dl.data_ptr(), K, sc["fmt"], rows_out=dr.data_ptr(), on_device=True)
    torch.cuda.synchronize()
    assert none is None and res3.as_dict() == wres
    S.assert_rows_equal(P, dr.cpu().numpy().view(P.REGION_SHAPE_DTYPE), wrows)


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
            rc, rows, res = gpu_shapes(P, gpu_ctx, sc["fmt"], depth, lab, K, where, layout)
            assert rc == P.ERR_ARG
            assert (rows.view(np.uint32) == PREFILL).all() and res.as_dict() == dict(n_regions=7, n_nonempty=7, n_labelled=7, n_clamped=7)
        # and the context still answers
        check(P, gpu_ctx, sc, (1, width, height, depth_kind), where, layout)


def test_argument_errors(P, gpu_ctx):
    lib = gpu_ctx.lib
    sc = R.scene(P, 1, 3, 2, "u16")
    fmt, K = R.with_color(P, sc["fmt"], "rgb8"), sc["n_regions"]
    d, l = sc["depth"], sc["labels"]
    rows = np.zeros(K, P.REGION_SHAPE_DTYPE)
    for on_dev in (0, 1):      # (every one of these is refused before a buffer is looked at: host pointers do for both forms)
        good = [gpu_ctx.handle, ctypes.byref(fmt), d.ctypes.data, l.ctypes.data, K, on_dev, rows.ctypes.data, on_dev, None]
        for k in (0, 1, 2, 3, 6):
            a = list(good); a[k] = None
            assert lib.f3ds_region_shapes(*a) == P.ERR_ARG, k
        for fields in (dict(width=0), dict(depth_type=7), dict(fx=0.0), dict(fy=float("nan")), dict(depth_scale=0.0), dict(cx=float("inf")), dict(depth_pitch=3)):
            f = fmt.copy()
            for k, v in fields.items():
                setattr(f, k, v)
            a = list(good); a[1] = ctypes.byref(f)
            assert lib.f3ds_region_shapes(*a) == P.ERR_ARG, fields
        a = list(good); a[4] = 0x01000000
        assert lib.f3ds_region_shapes(*a) == P.ERR_UNSUPPORTED
    # the colour fields are not looked at; n_regions == 0; a frame without a labelled pixel
    f = fmt.copy(); f.color_format = 99; f.color_pitch = 1
    res = P.RegionShapesResult()
    assert lib.f3ds_region_shapes(gpu_ctx.handle, ctypes.byref(f), d.ctypes.data, l.ctypes.data, K, 0, rows.ctypes.data, 0, ctypes.byref(res)) == 0
    S.assert_rows_equal(P, rows, S.ref_shapes(P, fmt, d, l, K)[1])
    none = np.full((2, 3), NO, np.uint32)
    assert lib.f3ds_region_shapes(gpu_ctx.handle, ctypes.byref(fmt), d.ctypes.data, none.ctypes.data, 0, 0, None, 0, ctypes.byref(res)) == 0
    assert res.as_dict() == dict(n_regions=0, n_nonempty=0, n_labelled=0, n_clamped=0)
    assert lib.f3ds_region_shapes(gpu_ctx.handle, ctypes.byref(fmt), d.ctypes.data, l.ctypes.data, 0, 0, None, 0, None) == P.ERR_ARG      # label 0 >= 0 regions
    rc, rows, res = gpu_shapes(P, gpu_ctx, fmt, np.zeros((2, 3), np.uint16), l, K)
    assert rc == 0 and res.as_dict() == dict(n_regions=K, n_nonempty=0, n_labelled=0, n_clamped=0)
    assert (S.words_of(rows) == np.array([0] + [R.QNAN] * 20, np.uint32)).all()


# ---- 3. end to end -----------------------------------------------------------------------------------------------------------------------------------------

def same(a, b):
    """two answers of a context (a tuple or a dict of arrays), byte for byte"""
    if isinstance(a, dict):
        a, b = [a[k] for k in sorted(a)], [b[k] for k in sorted(a)]
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_the_shapes_of_a_segmented_frame_and_the_context_afterwards(P):
    fmt, depth, color = frame_images(P, 7, 160, 120)
    prm = P.launch_params(voxel_res=0.02, seed_res=0.2)
    ctx, other = P.Context(0), P.Context(0)
    try:
        lab = ctx.segment_rgbd(depth, color, fmt, prm); K = int(ctx.result.n_regions)
        assert np.array_equal(other.segment_rgbd(depth, color, fmt, prm), lab) and K > 10
        rows, res = ctx.region_shapes(depth, lab, K, fmt)
        wrc, wrows, wres, _ = S.ref_shapes(P, fmt, depth, lab, K)
        assert wrc == 0 and res.as_dict() == wres
        S.assert_rows_equal(P, rows, wrows)
        assert int(rows["n_pixels"].astype(np.int64).sum()) == int((lab != NO).sum()) == res.n_labelled and 0 < res.n_nonempty <= K
        # the context answers as one that never made the call
        assert same(ctx.regions(), other.regions()) and same(ctx.voxel_cloud(), other.voxel_cloud())
        assert np.array_equal(ctx.recluster(prm), other.recluster(prm)) and ctx.result.n_regions == other.result.n_regions
        # one lower level of the same run
        levels, nreg = ctx.labels_at_thresholds([0.1])
        K1 = int(nreg[0])
        assert K1 >= K
        rows1, res1 = ctx.region_shapes(depth, levels[0], K1, fmt)
        wrows1, wres1 = S.ref_shapes(P, fmt, depth, levels[0], K1)[1:3]
        S.assert_rows_equal(P, rows1, wrows1)
        assert res1.as_dict() == wres1 and res1.n_labelled == res.n_labelled
        assert same(ctx.regions(), other.regions())
    finally:
        ctx.close(); other.close()


def test_rows_indexed_through_the_tracker(P, gpu_ctx):
    fmt, depth, color = frame_images(P, 7, 160, 120)
    prm = P.launch_params(voxel_res=0.02, seed_res=0.2)
    with P.Tracker(0, P.default_track_params(min_votes=1)) as trk:
        for _ in range(2):
            lab = gpu_ctx.segment_rgbd(depth, color, fmt, prm); K = int(gpu_ctx.result.n_regions)
            id_image = trk.update(depth, lab, K, fmt)
            rows, res = gpu_ctx.region_shapes(depth, lab, K, fmt)
            ids = trk.ids()
            valid = depth.reshape(-1) != 0
            count = np.bincount(id_image[valid & (id_image != NO)], minlength=int(trk.result.next_id))
            has = ids != NO
            assert len(ids) == K and has.sum() == res.n_nonempty and len(np.unique(ids[has])) == has.sum()
            assert np.array_equal(rows["n_pixels"][has], count[ids[has]]) and (rows["n_pixels"][~has] == 0).all() and count.sum() == res.n_labelled
