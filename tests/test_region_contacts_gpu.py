"""The region contacts on the device (f3ds_region_contacts: d_pair_init, d_contact_accum, the record sort, d_contact_finish: ContactRule of csrc/f3ds_contacts.inc over csrc/f3ds_pairs.inc)
against the numpy reference of tests/region_contacts_common.py, bit for bit: the scenes and shapes of tests/test_region_contacts_cpu.py, host buffers and
all-device buffers, at the default launch width and at F3DS_GRID_CAP = 1 and 3.  At one workgroup the 5917 pixels of 97 x 61 are one span of 23 full trips and
a ragged one; at three the spans end ragged and straddle rows, so lower neighbours fall into another workgroup's span.  Scene 3 (every pixel its own region)
has more than eleven thousand rows: forty times the 256 slots of the LDS table, more than the 2048 rows of the first download, and -- with
F3DS_RGC_FIRST_CAP = 4096, since 97 x 61 cannot reach the 32768 records of the first buffer -- more records than the first run has room for."""
import ctypes

import numpy as np
import pytest

import region_contacts_common as C
from region_contacts_common import NO
from rgbd_common import frame_images

pytestmark = pytest.mark.gpu
PREFILL = 0x5A5A5A5A
LDS_SLOTS, FIRST_ROWS, SHORT_FIRST_CAP = 256, 2048, 4096      # RGC_SLOTS and RGC_FIRST_ROWS of csrc/f3ds_contacts.inc; the short first record buffer of the tests
_refs = {}


def to_device(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
    torch.cuda.synchronize()
    return t


def reference(P, key, sc):
    """the numpy reference of a scene, computed once"""
    if key not in _refs:
        _refs[key] = C.ref_contacts(P, sc["fmt"], sc["depth"], sc["labels"], sc["n_regions"], sc["depth_tol"])
    return _refs[key]


def gpu_contacts(P, ctx, fmt, depth, labels, n_regions, depth_tol, where="host", layout="tight", cap=64, count_only=False):
    """f3ds_region_contacts on raw buffers: (rc, rows (all `cap` of them), n_out, result).  where "device": every buffer on the GPU.  The rows are prefilled
    with 0x5A5A5A5A words, n_out with 777, the result with sevens."""
    f, dbuf, _ = C.buffers(fmt, depth, None, layout)
    lab = np.ascontiguousarray(labels, np.uint32).reshape(-1)
    rows = np.full(8 * cap, PREFILL, np.uint32)
    res = P.RegionContactsResult(7, 7, 7, 7)
    n_out = ctypes.c_size_t(777)
    if where == "device":
        import torch
        dd, dl, dr = to_device(dbuf), to_device(lab.view(np.int32)), to_device(np.full(max(8 * cap, 1), PREFILL, np.uint32).view(np.int32))
        rc = ctx.lib.f3ds_region_contacts(ctx.handle, ctypes.byref(f), ctypes.c_void_p(dd.data_ptr()), ctypes.c_void_p(dl.data_ptr()), int(n_regions), depth_tol, 1,
                                          None if count_only else ctypes.c_void_p(dr.data_ptr()), cap, 1, ctypes.byref(n_out), ctypes.byref(res))
        torch.cuda.synchronize()
        rows = dr.cpu().numpy().view(np.uint32)[:8 * cap].copy()
    else:
        rc = ctx.lib.f3ds_region_contacts(ctx.handle, ctypes.byref(f), dbuf.ctypes.data, lab.ctypes.data, int(n_regions), depth_tol, 0,
                                          None if count_only else rows.ctypes.data, cap, 0, ctypes.byref(n_out), ctypes.byref(res))
    return rc, rows.view(P.REGION_CONTACT_DTYPE), n_out.value, res


def check(P, ctx, sc, key, where, layout):
    wrc, wrows, wres = reference(P, key, sc)
    n = len(wrows)
    rc, rows, n_out, res = gpu_contacts(P, ctx, sc["fmt"], sc["depth"], sc["labels"], sc["n_regions"], sc["depth_tol"], where, layout, cap=n + 2)
    assert rc == wrc == 0 and n_out == n
    C.assert_rows_equal(rows[:n], wrows, "%s %s" % (where, layout))
    assert (rows[n:].view(np.uint32) == PREFILL).all()                            # nothing behind the rows
    assert res.as_dict() == wres, (res.as_dict(), wres)
    return wrows, wres


# ---- 1. the scenes, every shape, default and narrow launches ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [0, 1, 3])
@pytest.mark.parametrize("which", C.SCENES)
@pytest.mark.parametrize("width,height,depth_kind,layout", C.SHAPES)
def test_scene_equals_numpy(P, gpu_ctx, monkeypatch, width, height, depth_kind, layout, which, cap):
    if cap:
        monkeypatch.setenv("F3DS_GRID_CAP", str(cap))
    if which == 3:
        monkeypatch.setenv("F3DS_RGC_FIRST_CAP", str(SHORT_FIRST_CAP))
    sc = C.scene(P, which, width, height, depth_kind)
    for where in ("host", "device"):
        rows, res = check(P, gpu_ctx, sc, (which, width, height, depth_kind), where, layout)
    if which == 3 and width * height > 5000:
        assert len(rows) > 10 * LDS_SLOTS and len(rows) > SHORT_FIRST_CAP and len(rows) > FIRST_ROWS
    if which == 2:
        assert len(rows) == 0


@pytest.mark.parametrize("seed", C.RANDOM_SEEDS)
def test_random_scene(P, gpu_ctx, monkeypatch, seed):
    if seed % 3 == 2:
        monkeypatch.setenv("F3DS_GRID_CAP", "1" if seed % 6 == 2 else "3")
    if seed % 4 == 1:
        monkeypatch.setenv("F3DS_RGC_FIRST_CAP", "16")                              # an ordinary frame that has to run twice
    sc, layout = C.random_case(P, seed)
    check(P, gpu_ctx, sc, ("random", seed), "device" if seed % 3 == 1 else "host", layout)


def test_package_method(P, gpu_ctx):
    sc = C.scene(P, 1, 97, 61, "u16")
    K = sc["n_regions"]
    wrows, wres = C.ref_contacts(P, sc["fmt"], sc["depth"], sc["labels"], K, 0.05)[1:]
    rows, res = gpu_ctx.region_contacts(sc["depth"], sc["labels"], K, sc["fmt"])
    C.assert_rows_equal(rows, wrows)
    assert res.as_dict() == wres and rows.dtype == P.REGION_CONTACT_DTYPE
    out = np.zeros(len(wrows) + 3, P.REGION_CONTACT_DTYPE)
    got = gpu_ctx.region_contacts(sc["depth"], sc["labels"], K, sc["fmt"], depth_tol=0.2, rows_out=out)[0]
    assert got.base is out and len(got) == len(wrows)
    C.assert_rows_equal(got, C.ref_contacts(P, sc["fmt"], sc["depth"], sc["labels"], K, 0.2)[1])
    with pytest.raises(P.F3dsError):
        gpu_ctx.region_contacts(sc["depth"], sc["labels"], K, sc["fmt"], rows_out=np.zeros(2, P.REGION_CONTACT_DTYPE))
    # more rows than the package's first buffer: grown from the count and repeated
    sc3 = C.scene(P, 3, 67, 45, "u16")
    rows3, res3 = gpu_ctx.region_contacts(sc3["depth"], sc3["labels"], sc3["n_regions"], sc3["fmt"])
    C.assert_rows_equal(rows3, C.ref_contacts(P, sc3["fmt"], sc3["depth"], sc3["labels"], sc3["n_regions"], 0.05)[1])
    assert res3.n_contacts == len(rows3) > FIRST_ROWS
    # device pointers through the package
    import torch
    dd, dl = to_device(sc["depth"].view(np.uint8)), to_device(sc["labels"].view(np.int32))
    cap = len(wrows) + 1
    dr = torch.zeros(8 * cap, dtype=torch.int32, device="cuda")
    none, res4 = gpu_ctx.region_contacts(dd.data_ptr(), dl.data_ptr(), K, sc["fmt"], rows_out=(dr.data_ptr(), cap), on_device=True)
    torch.cuda.synchronize()
    assert none is None and res4.as_dict() == wres
    C.assert_rows_equal(dr.cpu().numpy().view(P.REGION_CONTACT_DTYPE)[:len(wrows)], wrows)
    assert gpu_ctx.region_contacts(dd.data_ptr(), dl.data_ptr(), K, sc["fmt"], on_device=True)[1].as_dict() == wres      # count only


# ---- 2. errors, the count-only call and the capacity, in both forms --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("where", ["host", "device"])
def test_a_bad_label_is_found_on_the_device_and_leaves_everything(P, gpu_ctx, monkeypatch, where, cap):
    if cap:
        monkeypatch.setenv("F3DS_GRID_CAP", str(cap))
    for width, height, depth_kind, layout in C.SHAPES:      # (1 x 1 too: a pixel without a neighbour)
        sc = C.scene(P, 1, width, height, depth_kind)
        K = sc["n_regions"]
        for at, value, invalid_depth in ((-1, K, False), (0, K + 5, False), (-1, 0xFFFFFFFE, True)):
            lab = sc["labels"].copy(); lab.reshape(-1)[at] = value
            depth = sc["depth"].copy()
            if invalid_depth:
                depth.reshape(-1)[at] = 0
            rc, rows, n_out, res = gpu_contacts(P, gpu_ctx, sc["fmt"], depth, lab, K, 0.05, where, layout)
            assert rc == P.ERR_ARG
            assert (rows.view(np.uint32) == PREFILL).all() and n_out == 777 and res.as_dict() == dict(n_regions=7, n_contacts=7, n_pairs=7, n_close=7)
        # and the context still answers
        check(P, gpu_ctx, sc, (1, width, height, depth_kind), where, layout)


@pytest.mark.parametrize("where", ["host", "device"])
def test_count_only_and_capacity(P, gpu_ctx, where):
    sc = C.scene(P, 1, 97, 61, "u16")
    wrows, wres = reference(P, (1, 97, 61, "u16"), sc)[1:]
    n = len(wrows)
    args = (P, gpu_ctx, sc["fmt"], sc["depth"], sc["labels"], sc["n_regions"], sc["depth_tol"], where, "tight")
    rc, rows, n_out, res = gpu_contacts(*args, cap=n + 5, count_only=True)
    assert rc == 0 and n_out == n and res.as_dict() == wres and (rows.view(np.uint32) == PREFILL).all()
    rc, rows, n_out, res = gpu_contacts(*args, cap=n - 1)
    assert rc == P.ERR_CAPACITY and n_out == n and res.as_dict() == wres and (rows.view(np.uint32) == PREFILL).all()
    rc, rows, n_out, res = gpu_contacts(*args, cap=n)
    assert rc == 0 and n_out == n
    C.assert_rows_equal(rows, wrows)


def test_argument_errors(P, gpu_ctx):
    lib = gpu_ctx.lib
    sc = C.scene(P, 1, 3, 2, "u16")
    fmt, K = sc["fmt"], sc["n_regions"]
    d, l = sc["depth"], sc["labels"]
    rows = np.zeros(16, P.REGION_CONTACT_DTYPE)
    n_out = ctypes.c_size_t(0)
    tol = ctypes.c_float(0.05)
    for on_dev in (0, 1):      # (every one of these is refused before a buffer is looked at: host pointers do for both forms)
        good = [gpu_ctx.handle, ctypes.byref(fmt), d.ctypes.data, l.ctypes.data, K, tol, on_dev, rows.ctypes.data, len(rows), on_dev, ctypes.byref(n_out), None]
        for k in (0, 1, 2, 3, 10):
            a = list(good); a[k] = None
            assert lib.f3ds_region_contacts(*a) == P.ERR_ARG, k
        for fields in (dict(width=0), dict(depth_type=7), dict(fx=0.0), dict(fy=float("nan")), dict(depth_scale=0.0), dict(cx=float("inf")), dict(depth_pitch=3)):
            f = fmt.copy()
            for k, v in fields.items():
                setattr(f, k, v)
            a = list(good); a[1] = ctypes.byref(f)
            assert lib.f3ds_region_contacts(*a) == P.ERR_ARG, fields
        for bad in (-0.01, float("nan"), float("inf")):
            a = list(good); a[5] = ctypes.c_float(bad)
            assert lib.f3ds_region_contacts(*a) == P.ERR_ARG, bad
        a = list(good); a[4] = 0x01000000
        assert lib.f3ds_region_contacts(*a) == P.ERR_UNSUPPORTED
    # the colour fields are not looked at; zero rows: no region, one region, no labelled pixel
    f = fmt.copy(); f.color_format = 99; f.color_pitch = 1
    rc, got, n, res = gpu_contacts(P, gpu_ctx, f, d, l, K, 0.05)
    want = C.ref_contacts(P, fmt, d, l, K, 0.05)[1]
    assert rc == 0 and n == len(want)
    C.assert_rows_equal(got[:n], want)
    none = np.full((2, 3), NO, np.uint32)
    rc, got, n, res = gpu_contacts(P, gpu_ctx, fmt, d, none, 0, 0.05)
    assert rc == 0 and n == 0 and res.as_dict() == dict(n_regions=0, n_contacts=0, n_pairs=0, n_close=0)
    assert gpu_contacts(P, gpu_ctx, fmt, d, l, 0, 0.05)[0] == P.ERR_ARG      # label 0 >= 0 regions
    rc, got, n, res = gpu_contacts(P, gpu_ctx, fmt, d, np.zeros((2, 3), np.uint32), 1, 0.05)
    assert rc == 0 and n == 0 and res.as_dict() == dict(n_regions=1, n_contacts=0, n_pairs=0, n_close=0)
    rc, got, n, res = gpu_contacts(P, gpu_ctx, fmt, np.zeros((2, 3), np.uint16), l, K, 0.05)
    assert rc == 0 and n == 0 and res.as_dict() == dict(n_regions=K, n_contacts=0, n_pairs=0, n_close=0)


# ---- 3. end to end -----------------------------------------------------------------------------------------------------------------------------------------

def same(a, b):
    """two answers of a context (a tuple or a dict of arrays), byte for byte"""
    if isinstance(a, dict):
        a, b = [a[k] for k in sorted(a)], [b[k] for k in sorted(a)]
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_the_contacts_of_a_segmented_frame_and_the_context_afterwards(P):
    fmt, depth, color = frame_images(P, 7, 160, 120)
    prm = P.launch_params(voxel_res=0.02, seed_res=0.2)
    ctx, other = P.Context(0), P.Context(0)
    try:
        lab = ctx.segment_rgbd(depth, color, fmt, prm); K = int(ctx.result.n_regions)
        assert np.array_equal(other.segment_rgbd(depth, color, fmt, prm), lab) and K > 10
        rows, res = ctx.region_contacts(depth, lab, K, fmt)
        wrc, wrows, wres = C.ref_contacts(P, fmt, depth, lab, K, 0.05)
        assert wrc == 0 and res.as_dict() == wres and len(rows) > 0
        C.assert_rows_equal(rows, wrows)
        # the context answers as one that never made the call
        assert same(ctx.regions(), other.regions()) and same(ctx.voxel_cloud(), other.voxel_cloud())
        assert np.array_equal(ctx.recluster(prm), other.recluster(prm)) and ctx.result.n_regions == other.result.n_regions
        # one lower level of the same run: finer regions, at least as many contact pairs
        levels, nreg = ctx.labels_at_thresholds([0.1])
        K1 = int(nreg[0])
        assert K1 >= K
        rows1, res1 = ctx.region_contacts(depth, levels[0], K1, fmt)
        wrows1, wres1 = C.ref_contacts(P, fmt, depth, levels[0], K1, 0.05)[1:]
        C.assert_rows_equal(rows1, wrows1)
        assert res1.as_dict() == wres1 and res1.n_pairs >= res.n_pairs
        assert same(ctx.regions(), other.regions())
    finally:
        ctx.close(); other.close()


def test_rows_indexed_through_the_tracker(P, gpu_ctx):
    fmt, depth, color = frame_images(P, 7, 160, 120)
    prm = P.launch_params(voxel_res=0.02, seed_res=0.2)
    with P.Tracker(0, P.default_track_params(min_votes=1)) as trk:
        for _ in range(2):
            lab = gpu_ctx.segment_rgbd(depth, color, fmt, prm); K = int(gpu_ctx.result.n_regions)
            trk.update(depth, lab, K, fmt)
            rows, res = gpu_ctx.region_contacts(depth, lab, K, fmt)
            ids = trk.ids()
            assert len(ids) == K and len(rows) > 0
            ia, ib = ids[rows["a"]], ids[rows["b"]]
            assert (ia != NO).all() and (ib != NO).all() and (ia != ib).all()      # a region in a contact has a labelled pixel, so an id of its own
