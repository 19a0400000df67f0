"""The six label-image calls on the device at frames wider than a workgroup: every case of tests/label_image_wide_common.py (its docstring has the shapes, the
scenes and the classes of control flow each case is for; tests/test_label_image_wide_cpu.py asserts that census and the references) through f3ds_region_table,
_shapes, _boxes, _contacts, _components and the tracker update, against the cached references, bit for bit as u32 words.  Every case runs at the default
launch width, at F3DS_GRID_CAP = 1 (some 40 000 pixels become about 150 trips of one workgroup and one loop over 48 or 40 tiles) and at F3DS_GRID_CAP = 2048 (as
many workgroups as the frame allows), with its inputs and outputs once in host memory and once in device memory (torch tensors).  The table runs with every
colour format on the 257- and 640-wide shapes and with one, in turn, elsewhere; contacts at depth_tol 0.05 and 1e30, components at 0.05 and inf, min_pixels 1
and, for the speckles, 3; the tracker runs first / same / permuted labels, is reset, and runs them again from device memory.

The context's launch shape (Context.launch_shape, F3DS_DBG_LAUNCH_SHAPE) holds the cap of grid_for(), not the grid of a launch: the test asserts the cap and,
from it, the census's workgroup counts."""
import numpy as np
import pytest

import label_image_wide_common as W
import region_boxes_common as B
import region_components_common as C
import region_contacts_common as CT
import region_shapes_common as S
import region_table_common as R
from label_image_wide_common import NO

pytestmark = pytest.mark.gpu
PREFILL = 0x5A5A5A5A
IDS = [c.id for c in W.CASES]


class Device:
    """a case's laid-out inputs on the device, and output buffers prefilled with 0x5A5A5A5A words"""

    def __init__(self, fr, colors=()):
        import torch
        self.torch = torch
        self.depth = self.put(fr["dbuf"])
        self.labels = self.put(fr["labels"].view(np.int32))
        self.permuted = self.put(fr["permuted"].view(np.int32))
        self.color = {ck: self.put(fr["color"][ck][2]) for ck in colors if ck is not None}
        torch.cuda.synchronize()

    def put(self, arr):
        return self.torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)).cuda()

    def out(self, words):
        t = self.torch.full((max(int(words), 1),), PREFILL, dtype=self.torch.int32, device="cuda")
        self.torch.cuda.synchronize()
        return t

    def get(self, t, dtype, count):
        self.torch.cuda.synchronize()
        return t.cpu().numpy().view(np.uint32)[:count * dtype.itemsize // 4].copy().view(dtype)

    def untouched(self, t):
        self.torch.cuda.synchronize()
        return bool((t.cpu().numpy().view(np.uint32) == PREFILL).all())


U32 = np.dtype(np.uint32)


def table(P, ctx, case, fr, dev, ck, where, labels=None):
    wrc, wrows, wres = W.reference(P, case, "table", ck)
    K = fr["K"]
    color, f, _ = fr["color"][ck]
    if where == "device":
        dr = dev.out(18 * K)
        _, res = ctx.region_table(dev.depth.data_ptr(), (dev.labels if labels is None else labels).data_ptr(), K, f, color=None if ck is None else dev.color[ck].data_ptr(),
                                  rows_out=dr.data_ptr(), on_device=True)
        rows = dev.get(dr, P.REGION_ROW_DTYPE, K)
    else:
        rows, res = ctx.region_table(W.depth_view(case, fr), fr["labels"] if labels is None else labels, K, R.with_color(P, fr["fmt"], ck), W.color_view(case, fr, ck))
    R.assert_rows_equal(P, rows, wrows, "table %s %s %s" % (case.id, ck, where))
    assert wrc == 0 and res.as_dict() == wres, (res.as_dict(), wres)


def shapes(P, ctx, case, fr, dev, where):
    _, _, wshapes, wres = W.reference(P, case, "boxes")
    K = fr["K"]
    if where == "device":
        dr = dev.out(21 * K)
        _, res = ctx.region_shapes(dev.depth.data_ptr(), dev.labels.data_ptr(), K, fr["f"], rows_out=dr.data_ptr(), on_device=True)
        rows = dev.get(dr, P.REGION_SHAPE_DTYPE, K)
    else:
        rows, res = ctx.region_shapes(W.depth_view(case, fr), fr["labels"], K, fr["fmt"])
    S.assert_rows_equal(P, rows, wshapes, "shapes %s %s" % (case.id, where))
    assert res.as_dict() == W.shapes_result(wres), (res.as_dict(), wres)


def boxes(P, ctx, case, fr, dev, where):
    wrc, wrows, wshapes, wres = W.reference(P, case, "boxes")
    K = fr["K"]
    if where == "device":
        dr, ds = dev.out(24 * K), dev.out(21 * K)
        _, _, res = ctx.region_boxes(dev.depth.data_ptr(), dev.labels.data_ptr(), K, fr["f"], B.TOL, rows_out=dr.data_ptr(), shapes_out=ds.data_ptr(), on_device=True)
        rows, shp = dev.get(dr, P.REGION_BOX_DTYPE, K), dev.get(ds, P.REGION_SHAPE_DTYPE, K)
    else:
        rows, shp, res = ctx.region_boxes(W.depth_view(case, fr), fr["labels"], K, fr["fmt"], B.TOL, shapes_out=True)
    B.assert_rows_equal(P, rows, wrows, "boxes %s %s" % (case.id, where))
    S.assert_rows_equal(P, shp, wshapes, "boxes' shapes %s %s" % (case.id, where))
    assert wrc == 0 and res.as_dict() == wres, (res.as_dict(), wres)


def contacts(P, ctx, case, fr, dev, tol, where):
    wrc, wrows, wres = W.reference(P, case, "contacts", tol)
    K = fr["K"]
    if where == "device":
        cap = len(wrows) + 3
        dr = dev.out(8 * cap)
        _, res = ctx.region_contacts(dev.depth.data_ptr(), dev.labels.data_ptr(), K, fr["f"], tol, rows_out=(dr.data_ptr(), cap), on_device=True)
        rows = dev.get(dr, P.REGION_CONTACT_DTYPE, len(wrows))
        assert (dev.get(dr, U32, 8 * cap)[8 * len(wrows):] == PREFILL).all()
    else:
        rows, res = ctx.region_contacts(W.depth_view(case, fr), fr["labels"], K, fr["fmt"], tol)
    CT.assert_rows_equal(rows, wrows, "contacts %s %s %s" % (case.id, tol, where))
    assert wrc == 0 and res.as_dict() == wres, (res.as_dict(), wres)


def components(P, ctx, case, fr, dev, tol, minpix, where):
    wrc, wimage, wrows, wres = W.reference(P, case, "components", tol, minpix)
    K = fr["K"]
    if where == "device":
        cap = len(wrows) + 3
        dc, dr = dev.out(fr["n"]), dev.out(3 * cap)
        _, _, res = ctx.region_components(dev.depth.data_ptr(), dev.labels.data_ptr(), K, fr["f"], tol, minpix, rows_out=(dr.data_ptr(), cap), comp_out=dc.data_ptr(), on_device=True)
        image, rows = dev.get(dc, U32, fr["n"]), dev.get(dr, P.REGION_COMPONENT_DTYPE, len(wrows))
        assert (dev.get(dr, U32, 3 * cap)[3 * len(wrows):] == PREFILL).all()
    else:
        image, rows, res = ctx.region_components(W.depth_view(case, fr), fr["labels"], K, fr["fmt"], tol, minpix)
    C.assert_same(image, rows, wimage, wrows, "components %s %s %d %s" % (case.id, tol, minpix, where))
    assert wrc == 0 and res.as_dict() == wres, (res.as_dict(), wres)


def track(P, trk, case, fr, dev, first=0, last=6):
    """updates first ... last - 1 of track_frames() on `trk`: the first three from host memory, then a reset, then three from device memory"""
    want = W.reference(P, case, "track")
    for k, ((labels, reset), (wrc, wimg, wids, wres)) in list(enumerate(zip(W.track_frames(fr), want)))[first:last]:
        if reset:
            trk.reset()
        if k >= 3:
            di = dev.out(fr["n"])
            trk.update(dev.depth.data_ptr(), (dev.permuted if labels is fr["permuted"] else dev.labels).data_ptr(), fr["K"], fr["f"], ids_out=di.data_ptr(), on_device=True)
            got = dev.get(di, U32, fr["n"])
        else:
            got = trk.update(W.depth_view(case, fr), labels, fr["K"], fr["fmt"])
        np.testing.assert_array_equal(got, wimg, "track ids %s update %d" % (case.id, k))
        assert wrc == 0 and np.array_equal(trk.ids(), wids)
        assert trk.result.as_dict() == wres, (k, trk.result.as_dict(), wres)


def need_device(P):
    if P.device_count() < 1:
        pytest.fail("GPU test selected but libf3ds sees no HIP device (no CPU fallback exists)")


@pytest.mark.parametrize("cap", W.CAPS)
@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_the_region_calls_equal_their_references(P, gpu_ctx, monkeypatch, case, cap):
    if cap:
        monkeypatch.setenv("F3DS_GRID_CAP", str(cap))
    fr = W.frame(P, case)
    dev = Device(fr, case.colors)
    for where in ("host", "device"):
        for ck in case.colors:
            table(P, gpu_ctx, case, fr, dev, ck, where)
        shapes(P, gpu_ctx, case, fr, dev, where)
        boxes(P, gpu_ctx, case, fr, dev, where)
        for tol in W.CONTACT_TOLS:
            contacts(P, gpu_ctx, case, fr, dev, tol, where)
        for tol in W.COMPONENT_TOLS:
            for minpix in case.min_pixels:
                components(P, gpu_ctx, case, fr, dev, tol, minpix, where)
    # the launch width these calls ran at, and from it the workgroups of the accumulate launches as the census counts them
    shape = gpu_ctx.launch_shape()
    assert shape == (cap or W.GRID_CAP, cap or W.GRID_CAP, 1)
    for trips in (W.LI_TRIPS, W.RGC_TRIPS):
        assert min(shape[0], W.accum_grid(case.n, trips, W.GRID_CAP)) == W.accum_grid(case.n, trips, cap)
    if cap == 1:
        assert W.accum_grid(case.n, W.LI_TRIPS, cap) == 1 and W.span_of(case.n, 1) >= case.n
    elif "wrap32" in case.classes:
        assert W.accum_grid(case.n, W.LI_TRIPS, cap) > W.rgt_copies(fr["K"]) == 32


@pytest.mark.parametrize("cap", W.CAPS)
@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_the_tracker_equals_its_reference(P, monkeypatch, case, cap):
    need_device(P)
    if cap:
        monkeypatch.setenv("F3DS_GRID_CAP", str(cap))
    fr = W.frame(P, case)
    with P.Tracker(0) as trk:
        track(P, trk, case, fr, Device(fr))


@pytest.mark.parametrize("where", ["host", "device"])
def test_a_label_out_of_range_in_the_last_pixel(P, gpu_ctx, where):
    """640 x 61, the label of the last pixel of the last row equal to n_regions: every call says F3DS_ERR_ARG, writes nothing, and the next call is exact"""
    case = W.BAD_LABEL_CASE
    fr = W.frame(P, case)
    K, n = fr["K"], fr["n"]
    bad = fr["labels"].copy(); bad[-1, -1] = K
    dev = Device(fr, case.colors)
    dbad = dev.put(bad.view(np.int32))
    dev.torch.cuda.synchronize()
    depth, dp, f, fmt, ck = W.depth_view(case, fr), dev.depth.data_ptr(), fr["f"], fr["fmt"], "rgba8"
    color, cf, _ = fr["color"][ck]

    def refused(call):
        with pytest.raises(P.F3dsError) as e:
            call()
        assert e.value.code == P.ERR_ARG

    def host_rows(dtype, count):
        return np.full(count * dtype.itemsize // 4, PREFILL, np.uint32).view(dtype)

    def clean(*bufs):
        for b in bufs:
            assert dev.untouched(b) if where == "device" else bool((np.ascontiguousarray(b).view(np.uint32) == PREFILL).all())

    if where == "device":
        a, b, c = dev.out(18 * K), dev.out(24 * K), dev.out(21 * K)
        refused(lambda: gpu_ctx.region_table(dp, dbad.data_ptr(), K, cf, color=dev.color[ck].data_ptr(), rows_out=a.data_ptr(), on_device=True))
        clean(a); table(P, gpu_ctx, case, fr, dev, ck, where)
        refused(lambda: gpu_ctx.region_shapes(dp, dbad.data_ptr(), K, f, rows_out=c.data_ptr(), on_device=True))
        clean(c); shapes(P, gpu_ctx, case, fr, dev, where)
        refused(lambda: gpu_ctx.region_boxes(dp, dbad.data_ptr(), K, f, B.TOL, rows_out=b.data_ptr(), shapes_out=c.data_ptr(), on_device=True))
        clean(b, c); boxes(P, gpu_ctx, case, fr, dev, where)
        d = dev.out(8 * 64)
        refused(lambda: gpu_ctx.region_contacts(dp, dbad.data_ptr(), K, f, 0.05, rows_out=(d.data_ptr(), 64), on_device=True))
        clean(d); contacts(P, gpu_ctx, case, fr, dev, 0.05, where)
        e, g = dev.out(n), dev.out(3 * 64)
        refused(lambda: gpu_ctx.region_components(dp, dbad.data_ptr(), K, f, 0.05, 1, rows_out=(g.data_ptr(), 64), comp_out=e.data_ptr(), on_device=True))
        clean(e, g); components(P, gpu_ctx, case, fr, dev, 0.05, 1, where)
    else:
        a, b, c = host_rows(P.REGION_ROW_DTYPE, K), host_rows(P.REGION_BOX_DTYPE, K), host_rows(P.REGION_SHAPE_DTYPE, K)
        refused(lambda: gpu_ctx.region_table(depth, bad, K, R.with_color(P, fmt, ck), W.color_view(case, fr, ck), rows_out=a))
        clean(a); table(P, gpu_ctx, case, fr, dev, ck, where)
        refused(lambda: gpu_ctx.region_shapes(depth, bad, K, fmt, rows_out=c))
        clean(c); shapes(P, gpu_ctx, case, fr, dev, where)
        refused(lambda: gpu_ctx.region_boxes(depth, bad, K, fmt, B.TOL, rows_out=b, shapes_out=c))
        clean(b, c); boxes(P, gpu_ctx, case, fr, dev, where)
        d = host_rows(P.REGION_CONTACT_DTYPE, 64)
        refused(lambda: gpu_ctx.region_contacts(depth, bad, K, fmt, 0.05, rows_out=d))
        clean(d); contacts(P, gpu_ctx, case, fr, dev, 0.05, where)
        g = host_rows(P.REGION_COMPONENT_DTYPE, 64)
        refused(lambda: gpu_ctx.region_components(depth, bad, K, fmt, 0.05, 1, rows_out=g))
        clean(g); components(P, gpu_ctx, case, fr, dev, 0.05, 1, where)
    # the tracker: a refused update changes nothing of its state
    with P.Tracker(0) as trk:
        track(P, trk, case, fr, dev, 0, 1)
        if where == "device":
            di = dev.out(n)
            refused(lambda: trk.update(dp, dbad.data_ptr(), K, f, ids_out=di.data_ptr(), on_device=True))
            clean(di)
        else:
            di = np.full(n, PREFILL, np.uint32)
            refused(lambda: trk.update(depth, bad, K, fmt, ids_out=di))
            clean(di)
        track(P, trk, case, fr, dev, 1, 6)
