"""The region components on the device (f3ds_region_components: d_comp_local, d_comp_seam, d_comp_flatten, d_comp_flag, the scan, d_comp_write in
csrc/f3ds_components.inc) against the reference of tests/region_components_common.py, bit for bit: the scenes and shapes of
tests/test_region_components_cpu.py, host buffers and all-device buffers, at the default launch width and at F3DS_GRID_CAP = 1 and 3.  97 x 61 is two by four
tiles of 64 x 16 pixels, ragged in both directions: at one workgroup it walks all eight, at three the tile loop ends unevenly.  Scene table3 (every pixel its
own region) has more than five thousand rows, more than the 2048 of the first download."""
import ctypes

import numpy as np
import pytest

import region_components_common as K
from region_components_common import NO
from rgbd_common import frame_images

pytestmark = pytest.mark.gpu
PREFILL = 0x5A5A5A5A
FIRST_ROWS = 2048      # RGK_FIRST_ROWS of csrc/f3ds_components.inc
SEVENS = dict(n_regions=7, n_components=7, n_dropped=7, reserved=7, n_labelled=7, n_kept=7)


def to_device(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
    torch.cuda.synchronize()
    return t


def gpu_components(P, ctx, sc, where="host", layout="tight", cap=64, no_rows=False, labels=None, depth=None, n_regions=None):
    """f3ds_region_components on raw buffers: (rc, image, rows (all `cap` of them), n_out, result).  where "device": every buffer on the GPU.  Image and rows
    are prefilled with 0x5A5A5A5A words, n_out with 777, the result with sevens."""
    f, dbuf, _ = K.buffers(sc["fmt"], sc["depth"] if depth is None else depth, None, layout)
    lab = np.ascontiguousarray(sc["labels"] if labels is None else labels, np.uint32).reshape(-1)
    nreg = int(sc["n_regions"] if n_regions is None else n_regions)
    prm = P.ComponentParams(sc["depth_tol"], sc["min_pixels"])
    h, w = int(f.height), int(f.width)
    image = np.full(h * w, PREFILL, np.uint32)
    rows = np.full(3 * cap, PREFILL, np.uint32)
    res = P.RegionComponentsResult(7, 7, 7, 7, 7, 7)
    n_out = ctypes.c_size_t(777)
    if where == "device":
        import torch
        dd, dl = to_device(dbuf), to_device(lab.view(np.int32))
        di, dr = to_device(image.view(np.int32)), to_device(np.full(max(3 * cap, 1), PREFILL, np.uint32).view(np.int32))
        rc = ctx.lib.f3ds_region_components(ctx.handle, ctypes.byref(f), ctypes.c_void_p(dd.data_ptr()), ctypes.c_void_p(dl.data_ptr()), nreg, ctypes.byref(prm), 1,
                                            ctypes.c_void_p(di.data_ptr()), None if no_rows else ctypes.c_void_p(dr.data_ptr()), cap, 1, ctypes.byref(n_out), ctypes.byref(res))
        torch.cuda.synchronize()
        image = di.cpu().numpy().view(np.uint32).copy()
        rows = dr.cpu().numpy().view(np.uint32)[:3 * cap].copy()
    else:
        rc = ctx.lib.f3ds_region_components(ctx.handle, ctypes.byref(f), dbuf.ctypes.data, lab.ctypes.data, nreg, ctypes.byref(prm), 0, image.ctypes.data,
                                            None if no_rows else rows.ctypes.data, cap, 0, ctypes.byref(n_out), ctypes.byref(res))
    return rc, image.reshape(h, w), rows.view(P.REGION_COMPONENT_DTYPE), n_out.value, res


def check(P, ctx, sc, key, where, layout):
    wrc, wimage, wrows, wres = K.reference(P, key, sc)
    n = len(wrows)
    rc, image, rows, n_out, res = gpu_components(P, ctx, sc, where, layout, cap=n + 2)
    assert rc == wrc == 0 and n_out == n
    K.assert_same(image, rows[:n], wimage, wrows, "%s %s %s" % (key, where, layout))
    assert (rows[n:].view(np.uint32) == PREFILL).all()                            # nothing behind the rows
    assert res.as_dict() == wres, (res.as_dict(), wres)
    return wimage, wrows, wres


# ---- 1. the scenes, every shape, default and narrow launches ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [0, 1, 3])
@pytest.mark.parametrize("name", K.SCENES)
def test_scene_equals_reference(P, gpu_ctx, monkeypatch, name, cap):
    if cap:
        monkeypatch.setenv("F3DS_GRID_CAP", str(cap))
    for width, height, depth_kind, layout in K.SHAPES:
        sc = K.scene(P, name, width, height, depth_kind)
        for where in ("host", "device"):
            image, rows, res = check(P, gpu_ctx, sc, (name, width, height, depth_kind), where, layout)
        if name == "table3" and width * height > 5000:
            assert len(rows) > FIRST_ROWS
        if name == "spiral" and min(width, height) >= 8:
            assert len(rows) == 2
        if name.startswith("comb") and min(width, height) >= 8:
            assert len(rows) == 1


@pytest.mark.parametrize("seed", K.RANDOM_SEEDS)
def test_random_scene(P, gpu_ctx, monkeypatch, seed):
    sc, layout, cap = K.random_case(P, seed)
    if cap:
        monkeypatch.setenv("F3DS_GRID_CAP", str(cap))
    check(P, gpu_ctx, sc, ("random", seed), "device" if seed % 3 == 1 else "host", layout)


# ---- 2. properties -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["table1", "spiral", "comb_right", "stripes", "speckles"])
def test_the_components_of_the_component_image_are_the_identity(P, gpu_ctx, name):
    for width, height, depth_kind, layout in K.SHAPES[:2]:
        sc = K.scene(P, name, width, height, depth_kind)
        rc, image, rows, n, res = gpu_components(P, gpu_ctx, sc, "host", layout, cap=width * height)
        again = dict(sc, labels=image, n_regions=n)
        rc2, image2, rows2, n2, res2 = gpu_components(P, gpu_ctx, again, "device", layout, cap=width * height)
        assert rc == rc2 == 0 and n2 == n and image2.tobytes() == image.tobytes()
        rows, rows2 = rows[:n], rows2[:n]
        assert np.array_equal(rows2["region"], np.arange(n)) and np.array_equal(rows2["first_pixel"], rows["first_pixel"]) and np.array_equal(rows2["n_pixels"], rows["n_pixels"])
        assert res2.n_dropped == 0 and res2.n_labelled == res.n_kept


@pytest.mark.parametrize("name", ["table1", "table6", "occluder", "stripes", "speckles"])
def test_the_table_and_the_contacts_of_the_component_image(P, gpu_ctx, name):
    for width, height, depth_kind, layout in K.SHAPES[:2]:
        sc = K.scene(P, name, width, height, depth_kind)
        image, rows, res = gpu_ctx.region_components(sc["depth"], sc["labels"], sc["n_regions"], sc["fmt"], depth_tol=sc["depth_tol"], min_pixels=sc["min_pixels"])
        n = res.n_components
        trows, tres = gpu_ctx.region_table(sc["depth"], image, n, sc["fmt"])
        assert np.array_equal(trows["n_pixels"], rows["n_pixels"]) and np.array_equal(trows["first_pixel"], rows["first_pixel"]) and tres.n_nonempty == n
        crows, cres = gpu_ctx.region_contacts(sc["depth"], image, n, sc["fmt"], depth_tol=sc["depth_tol"])
        same_region = rows["region"][crows["a"]] == rows["region"][crows["b"]]
        assert (crows["n_close"][same_region] == 0).all()                             # otherwise they would be one component
        if name == "stripes":
            assert same_region.any()


def test_package_method(P, gpu_ctx):
    sc = K.scene(P, "occluder", 97, 61, "u16")
    nreg = sc["n_regions"]
    wimage, wrows, wres = K.ref_components(P, sc["fmt"], sc["depth"], sc["labels"], nreg)[1:]
    image, rows, res = gpu_ctx.region_components(sc["depth"], sc["labels"], nreg, sc["fmt"])
    K.assert_same(image, rows, wimage, wrows)
    assert res.as_dict() == wres and rows.dtype == P.REGION_COMPONENT_DTYPE and image.shape == (61, 97)
    out = np.zeros(len(wrows) + 3, P.REGION_COMPONENT_DTYPE)
    got = gpu_ctx.region_components(sc["depth"], sc["labels"], nreg, sc["fmt"], depth_tol=K.INF, rows_out=out)[1]
    assert got.base is out and len(got) == len(wrows)
    with pytest.raises(P.F3dsError):
        gpu_ctx.region_components(sc["depth"], sc["labels"], nreg, sc["fmt"], rows_out=np.zeros(2, P.REGION_COMPONENT_DTYPE))
    sp = K.scene(P, "speckles", 97, 61, "u16")
    image2, rows2, res2 = gpu_ctx.region_components(sp["depth"], sp["labels"], sp["n_regions"], sp["fmt"], min_pixels=3)
    K.assert_same(image2, rows2, *K.ref_components(P, sp["fmt"], sp["depth"], sp["labels"], sp["n_regions"], 0.05, 3)[1:3])
    # more rows than the package's first buffer: grown from the count and repeated
    sc3 = K.scene(P, "table3", 67, 45, "u16")
    image3, rows3, res3 = gpu_ctx.region_components(sc3["depth"], sc3["labels"], sc3["n_regions"], sc3["fmt"])
    K.assert_same(image3, rows3, *K.ref_components(P, sc3["fmt"], sc3["depth"], sc3["labels"], sc3["n_regions"])[1:3])
    assert res3.n_components == len(rows3) > FIRST_ROWS
    # device pointers through the package
    import torch
    dd, dl = to_device(sc["depth"].view(np.uint8)), to_device(sc["labels"].view(np.int32))
    cap = len(wrows) + 1
    di = torch.zeros(97 * 61, dtype=torch.int32, device="cuda")
    dr = torch.zeros(3 * cap, dtype=torch.int32, device="cuda")
    none, none2, res4 = gpu_ctx.region_components(dd.data_ptr(), dl.data_ptr(), nreg, sc["fmt"], rows_out=(dr.data_ptr(), cap), comp_out=di.data_ptr(), on_device=True)
    torch.cuda.synchronize()
    assert none is None and none2 is None and res4.as_dict() == wres
    K.assert_same(di.cpu().numpy().view(np.uint32), dr.cpu().numpy().view(P.REGION_COMPONENT_DTYPE)[:len(wrows)], wimage, wrows)
    assert gpu_ctx.region_components(dd.data_ptr(), dl.data_ptr(), nreg, sc["fmt"], comp_out=di.data_ptr(), on_device=True)[2].as_dict() == wres      # no rows


# ---- 3. errors, the call without rows and the capacity, in both forms ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("where", ["host", "device"])
def test_a_bad_label_is_found_on_the_device_and_leaves_everything(P, gpu_ctx, monkeypatch, where, cap):
    if cap:
        monkeypatch.setenv("F3DS_GRID_CAP", str(cap))
    for width, height, depth_kind, layout in K.SHAPES:      # (1 x 1 too)
        sc = K.scene(P, "table1", width, height, depth_kind)
        nreg = sc["n_regions"]
        for at, value, invalid_depth in ((-1, nreg, False), (0, nreg + 5, False), (-1, 0xFFFFFFFE, True)):
            lab = sc["labels"].copy(); lab.reshape(-1)[at] = value
            depth = sc["depth"].copy()
            if invalid_depth:
                depth.reshape(-1)[at] = 0
            rc, image, rows, n_out, res = gpu_components(P, gpu_ctx, sc, where, layout, labels=lab, depth=depth)
            assert rc == P.ERR_ARG
            assert (image == PREFILL).all() and (rows.view(np.uint32) == PREFILL).all() and n_out == 777 and res.as_dict() == SEVENS
        # and the context still answers
        check(P, gpu_ctx, sc, ("table1", width, height, depth_kind), where, layout)


@pytest.mark.parametrize("where", ["host", "device"])
def test_no_rows_and_capacity(P, gpu_ctx, where):
    sc = K.scene(P, "table1", 97, 61, "u16")
    wimage, wrows, wres = K.reference(P, ("table1", 97, 61, "u16"), sc)[1:]
    n = len(wrows)
    assert n > 3
    rc, image, rows, n_out, res = gpu_components(P, gpu_ctx, sc, where, cap=n + 5, no_rows=True)      # rows == NULL: cap is ignored, the image is written
    assert rc == 0 and n_out == n and res.as_dict() == wres and (rows.view(np.uint32) == PREFILL).all() and np.array_equal(image, wimage)
    rc, image, rows, n_out, res = gpu_components(P, gpu_ctx, sc, where, cap=n - 1)                     # too small: no row; the image, the count and the result are written
    assert rc == P.ERR_CAPACITY and n_out == n and res.as_dict() == wres and (rows.view(np.uint32) == PREFILL).all() and np.array_equal(image, wimage)
    rc, image, rows, n_out, res = gpu_components(P, gpu_ctx, sc, where, cap=n)
    assert rc == 0 and n_out == n
    K.assert_same(image, rows, wimage, wrows)


def test_argument_errors(P, gpu_ctx):
    lib = gpu_ctx.lib
    sc = K.scene(P, "table1", 3, 2, "u16")
    fmt, nreg = sc["fmt"], sc["n_regions"]
    d, l = sc["depth"], sc["labels"]
    image = np.zeros(6, np.uint32)
    rows = np.zeros(16, P.REGION_COMPONENT_DTYPE)
    n_out = ctypes.c_size_t(0)
    prm = P.ComponentParams(0.05, 1)
    for on_dev in (0, 1):      # (every one of these is refused before a buffer is looked at: host pointers do for both forms)
        good = [gpu_ctx.handle, ctypes.byref(fmt), d.ctypes.data, l.ctypes.data, nreg, ctypes.byref(prm), on_dev, image.ctypes.data, rows.ctypes.data, len(rows), on_dev,
                ctypes.byref(n_out), None]
        for k in (0, 1, 2, 3, 7, 11):
            a = list(good); a[k] = None
            assert lib.f3ds_region_components(*a) == P.ERR_ARG, k
        a = list(good); a[7] = l.ctypes.data                                          # comp_labels == labels
        assert lib.f3ds_region_components(*a) == P.ERR_ARG
        for fields in (dict(width=0), dict(depth_type=7), dict(fx=0.0), dict(fy=float("nan")), dict(depth_scale=0.0), dict(cx=float("inf")), dict(depth_pitch=3)):
            f = fmt.copy()
            for k, v in fields.items():
                setattr(f, k, v)
            a = list(good); a[1] = ctypes.byref(f)
            assert lib.f3ds_region_components(*a) == P.ERR_ARG, fields
        for bad in (-0.01, float("nan"), -float("inf")):
            p2 = P.ComponentParams(bad, 1)
            a = list(good); a[5] = ctypes.byref(p2)
            assert lib.f3ds_region_components(*a) == P.ERR_ARG, bad
        a = list(good); a[4] = 0x01000000
        assert lib.f3ds_region_components(*a) == P.ERR_UNSUPPORTED
    # NULL params are the defaults; the colour fields are not looked at; zero components: no region, no labelled pixel, a 1 x 1 image
    want = K.ref_components(P, fmt, d, l, nreg)
    good = [gpu_ctx.handle, ctypes.byref(fmt), d.ctypes.data, l.ctypes.data, nreg, None, 0, image.ctypes.data, rows.ctypes.data, len(rows), 0, ctypes.byref(n_out), None]
    assert lib.f3ds_region_components(*good) == 0 and n_out.value == len(want[2])
    K.assert_same(image, rows[:n_out.value], want[1], want[2])
    sc2 = dict(sc, fmt=fmt.copy()); sc2["fmt"].color_format = 99; sc2["fmt"].color_pitch = 1
    rc, got, grows, n, res = gpu_components(P, gpu_ctx, sc2)
    assert rc == 0 and n == len(want[2]) and np.array_equal(got, want[1])
    zero = dict(n_components=0, n_dropped=0, reserved=0, n_labelled=0, n_kept=0)
    none = np.full((2, 3), NO, np.uint32)
    rc, got, grows, n, res = gpu_components(P, gpu_ctx, sc, labels=none, n_regions=0)
    assert rc == 0 and n == 0 and res.as_dict() == dict(zero, n_regions=0) and (got == NO).all()
    assert gpu_components(P, gpu_ctx, sc, n_regions=0)[0] == P.ERR_ARG      # label 0 >= 0 regions
    rc, got, grows, n, res = gpu_components(P, gpu_ctx, sc, depth=np.zeros((2, 3), np.uint16))
    assert rc == 0 and n == 0 and res.as_dict() == dict(zero, n_regions=nreg) and (got == NO).all()
    sc1 = K.scene(P, "table2", 1, 1, "f32")
    for where in ("host", "device"):
        rc, got, grows, n, res = gpu_components(P, gpu_ctx, sc1, where)
        assert rc == 0 and n == 1 and got[0, 0] == 0 and tuple(grows[0]) == (0, 0, 1)
        rc, got, grows, n, res = gpu_components(P, gpu_ctx, sc1, where, labels=np.full((1, 1), NO, np.uint32))
        assert rc == 0 and n == 0 and got[0, 0] == NO and res.as_dict() == dict(zero, n_regions=1)


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------------------------------

def same(a, b):
    """two answers of a context (a tuple or a dict of arrays), byte for byte"""
    if isinstance(a, dict):
        a, b = [a[k] for k in sorted(a)], [b[k] for k in sorted(a)]
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_the_components_of_a_segmented_frame_the_tracker_and_the_context_afterwards(P):
    fmt, depth, color = frame_images(P, 7, 160, 120)
    prm = P.launch_params(voxel_res=0.02, seed_res=0.2)
    ctx, other = P.Context(0), P.Context(0)
    try:
        lab = ctx.segment_rgbd(depth, color, fmt, prm); nreg = int(ctx.result.n_regions)
        assert np.array_equal(other.segment_rgbd(depth, color, fmt, prm), lab) and nreg > 10
        image, rows, res = ctx.region_components(depth, lab, nreg, fmt)
        wrc, wimage, wrows, wres = K.ref_components(P, fmt, depth, lab, nreg)
        assert wrc == 0 and res.as_dict() == wres and len(rows) >= int(np.unique(np.asarray(lab).reshape(image.shape)[image != NO]).size)
        K.assert_same(image, rows, wimage, wrows)
        # the tracker takes the component image as any label image: every component with a pixel gets an id of its own, and keeps it on the same frame again
        with P.Tracker(0, P.default_track_params(min_votes=1)) as trk:
            trk.update(depth, image, res.n_components, fmt)
            ids = trk.ids().copy()
            assert len(ids) == res.n_components and (ids != NO).all() and len(set(ids.tolist())) == len(ids)
            image_b, rows_b, res_b = ctx.region_components(depth, lab, nreg, fmt)
            assert image_b.tobytes() == image.tobytes()
            trk.update(depth, image_b, res_b.n_components, fmt)
            ids_b = trk.ids()
            assert len(ids_b) == res.n_components and (ids_b != NO).all() and len(set(ids_b.tolist())) == len(ids_b)
        # the context answers as one that never made the call
        assert same(ctx.regions(), other.regions()) and same(ctx.voxel_cloud(), other.voxel_cloud())
        assert np.array_equal(ctx.recluster(prm), other.recluster(prm)) and ctx.result.n_regions == other.result.n_regions
        # with min_pixels the speckles go: fewer components, the same labelled pixels
        image2, rows2, res2 = ctx.region_components(depth, lab, nreg, fmt, min_pixels=20)
        K.assert_same(image2, rows2, *K.ref_components(P, fmt, depth, lab, nreg, 0.05, 20)[1:3])
        assert res2.n_components <= res.n_components and res2.n_labelled == res.n_labelled and res2.n_components + res2.n_dropped == res.n_components
        assert same(ctx.regions(), other.regions())
    finally:
        ctx.close(); other.close()
