"""The batch forms of the five region calls on the device (f3ds_region_table_batch, _shapes_batch, _boxes_batch, _contacts_batch, _components_batch) against
the f3ds_*_host functions, frame by frame and bit for bit: the batches of tests/region_batch_common.py for all five calls, from host and from device buffers, at
the default launch width and at F3DS_GRID_CAP = 1 and 3, every output prefilled with 0x5A5A5A5A words; then the launch shape, a bad label in one frame, a
capacity one row short, the contacts' overflow and rerun, the refusals of the call as a whole, lone and batch calls interleaved on the same contexts, and the
five batch calls behind f3ds_segment_rgbd_batch."""
import ctypes

import numpy as np
import pytest

import region_batch_common as C
from region_batch_common import UNSET
from rgbd_common import frame_images

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs(P):
    """five contexts for the whole file: the batches run on the first nctx of them, in every order of sizes"""
    if P.device_count() < 1:
        pytest.fail("GPU test selected but libf3ds sees no HIP device (no CPU fallback exists)")
    pool = [P.Context(0) for _ in range(5)]
    yield pool
    for c in pool:
        c.close()


def of(ctxs, B):
    return ctxs[:B.nctx]


# ---- 1. the batches, all five calls, both forms, default and narrow launches -------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [0, 1, 3])
@pytest.mark.parametrize("name", C.BATCHES)
@pytest.mark.parametrize("call", C.CALLS)
def test_batch_equals_the_host_functions(P, ctxs, monkeypatch, call, name, cap):
    if cap:
        monkeypatch.setenv("F3DS_GRID_CAP", str(cap))
    B = C.batch(P, name)
    for where in ("host", "device"):
        for color_kind in (["rgb8", "rgba8", "packed", None] if call == "table" else [None]):
            out = C.run(P, of(ctxs, B), B, call, where, color_kind=color_kind)
            C.assert_batch(P, B, call, out, "%s cap %d colour %s" % (where, cap, color_kind), color_kind=color_kind)
            for c in of(ctxs, B):
                assert c.launch_shape()[2] == B.nctx      # one launch for the batch, not a loop of lone calls
    if name == "four" and call in ("contacts", "components"):
        assert C.row_count(P, B, 1, call) > C.FIRST_ROWS      # (scene 3: more rows than ride with the head)
    if name == "five" and call == "table":
        assert C.reference(P, B, 4, "table")[2].n_clamped > 0 and C.reference(P, B, 1, "table")[2].n_labelled == 0


def test_the_batch_of_one_is_the_lone_call(P, ctxs):
    B = C.batch(P, "one")
    fr = B.frames[0]
    ctx = ctxs[0]
    rows, res = ctx.region_table(fr["depth"], fr["labels"], fr["K"], B.fmt)
    (brows, bres), = P.region_table_batch([ctx], [fr["depth"]], [fr["labels"]], [fr["K"]], B.fmt)[0]
    assert rows.tobytes() == brows.tobytes() and res.as_dict() == bres.as_dict()
    rows, shapes, res = ctx.region_boxes(fr["depth"], fr["labels"], fr["K"], B.fmt, shapes_out=True)
    (brows, bshapes, bres), = P.region_boxes_batch([ctx], [fr["depth"]], [fr["labels"]], [fr["K"]], B.fmt, shapes_out=True)[0]
    assert rows.tobytes() == brows.tobytes() and shapes.tobytes() == bshapes.tobytes() and res.as_dict() == bres.as_dict()
    image, rows, res = ctx.region_components(fr["depth"], fr["labels"], fr["K"], B.fmt)
    (bimage, brows, bres), = P.region_components_batch([ctx], [fr["depth"]], [fr["labels"]], [fr["K"]], B.fmt)[0]
    assert image.tobytes() == bimage.tobytes() and rows.tobytes() == brows.tobytes() and res.as_dict() == bres.as_dict()


def test_package_functions(P, ctxs):
    """the module-level functions in the host form: every frame equals the Context method, rows beyond the package's first buffer included (scene 3)"""
    B = C.batch(P, "four")
    cs = of(ctxs, B)
    d, l, k = [f["depth"] for f in B.frames], [f["labels"] for f in B.frames], [f["K"] for f in B.frames]
    colors = [C.color_of(B, i, "rgba8") for i in range(B.nctx)]
    fc = C.R.with_color(P, B.fmt, "rgba8")
    for name, kw, lone_kw in (("table", dict(colors=colors), [dict(color=c) for c in colors]), ("shapes", {}, None), ("boxes", dict(shapes_out=True), None),
                              ("contacts", {}, None), ("components", dict(min_pixels=2), None)):
        fmt = fc if name == "table" else B.fmt
        frames, status = getattr(P, "region_%s_batch" % name)(cs, d, l, k, fmt, **kw)
        assert status.dtype == np.int32 and (status == 0).all() and len(frames) == B.nctx
        for i, c in enumerate(cs):
            one_kw = lone_kw[i] if lone_kw else kw
            want = getattr(c, "region_" + name)(d[i], l[i], k[i], fmt, **one_kw)
            assert len(frames[i]) == len(want)
            for g, w in zip(frames[i], want):
                if isinstance(w, np.ndarray):
                    assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, i)
                else:
                    assert g.as_dict() == w.as_dict(), (name, i)
    # a caller's buffer one row short: that frame's status, not an exception; the others complete
    n1 = C.row_count(P, B, 0, "contacts")
    outs = [np.zeros(n1 - 1, P.REGION_CONTACT_DTYPE), None, None, None]
    frames, status = P.region_contacts_batch(cs, d, l, k, B.fmt, rows_out=outs)
    assert status.tolist() == [P.ERR_CAPACITY, 0, 0, 0] and frames[0][0] is None and frames[0][1].n_contacts == n1 and len(frames[1][0]) == C.row_count(P, B, 1, "contacts")
    # a bad label: returned, not raised
    bad = [x.copy() for x in l]; bad[2].reshape(-1)[100] = k[2]
    frames, status = P.region_shapes_batch(cs, d, bad, k, B.fmt)
    assert status.tolist() == [0, 0, P.ERR_ARG, 0] and frames[2] == (None, None) and frames[3][0].tobytes() == C.reference(P, B, 3, "shapes")[1].tobytes()
    # the call as a whole refused: raised
    with pytest.raises(P.F3dsError):
        P.region_shapes_batch([cs[0], cs[0]], d[:2], l[:2], k[:2], B.fmt)


def test_device_form_through_the_package(P, ctxs):
    import torch
    B = C.batch(P, "four")
    cs = of(ctxs, B)
    dd = [torch.from_numpy(f["depth"].view(np.uint8).reshape(-1).copy()).cuda() for f in B.frames]
    dl = [torch.from_numpy(f["labels"].view(np.int32).reshape(-1).copy()).cuda() for f in B.frames]
    k = [f["K"] for f in B.frames]
    rows = [torch.zeros(max(21 * x, 1), dtype=torch.int32, device="cuda") for x in k]
    torch.cuda.synchronize()
    frames, status = P.region_shapes_batch(cs, dd, dl, k, B.fmt, rows_out=rows, on_device=True)
    torch.cuda.synchronize()
    assert (status == 0).all()
    for i in range(B.nctx):
        want = C.reference(P, B, i, "shapes")
        assert frames[i][0] is None and frames[i][1].as_dict() == want[2].as_dict()
        assert rows[i].cpu().numpy().view(np.uint32)[:21 * k[i]].tobytes() == want[1].tobytes()
    caps = [C.row_count(P, B, i, "components") + 1 for i in range(B.nctx)]
    comp = [torch.zeros(B.n, dtype=torch.int32, device="cuda") for _ in k]
    crow = [torch.zeros(3 * c, dtype=torch.int32, device="cuda") for c in caps]
    torch.cuda.synchronize()
    frames, status = P.region_components_batch(cs, dd, dl, k, B.fmt, rows_out=[(r.data_ptr(), c) for r, c in zip(crow, caps)], comp_out=comp, on_device=True)
    torch.cuda.synchronize()
    assert (status == 0).all()
    for i in range(B.nctx):
        want = C.reference(P, B, i, "components")
        assert frames[i][2].as_dict() == want[3].as_dict() and comp[i].cpu().numpy().view(np.uint32).tobytes() == want[1].tobytes()
        assert crow[i].cpu().numpy().view(np.uint32)[:3 * len(want[2])].tobytes() == want[2].tobytes()


# ---- 2. per-frame outcomes -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("call", C.CALLS)
def test_a_bad_label_fails_its_frame_alone(P, ctxs, monkeypatch, call, where, cap):
    if cap:
        monkeypatch.setenv("F3DS_GRID_CAP", str(cap))
    B = C.batch(P, "four")
    mid = 2      # (scene 2: one region, so label 1 is out of range)
    lab = B.frames[mid]["labels"].copy(); lab.reshape(-1)[B.n // 2 + 5] = B.frames[mid]["K"]
    caps = [C.row_count(P, B, i, call) + 2 for i in range(B.nctx)] if call in ("contacts", "components") else None
    out = C.run(P, of(ctxs, B), B, call, where, labels={mid: lab}, caps=caps)
    assert out["rc"] == P.ERR_ARG and out["status"].tolist() == [0, 0, P.ERR_ARG, 0]
    assert C.untouched(P, call, out["frames"][mid])
    for i in (0, 1, 3):
        C.assert_frame(P, call, out["frames"][i], C.reference(P, B, i, call), "frame %d beside a bad label" % i)
    assert C.reference(P, B, mid, call, labels=lab) == ("arg",)      # (the definition refuses it too)
    # and the contexts still answer lone calls
    for i, c in enumerate(of(ctxs, B)):
        fr = B.frames[i]
        rows, res = c.region_shapes(fr["depth"], fr["labels"], fr["K"], B.fmt)
        assert rows.tobytes() == C.reference(P, B, i, "shapes")[1].tobytes()


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("call", ["contacts", "components"])
def test_a_capacity_one_row_short_fails_its_frame_alone(P, ctxs, call, where):
    B = C.batch(P, "four")
    counts = [C.row_count(P, B, i, call) for i in range(B.nctx)]
    for short in (0, 1):      # (frame 1 has more rows than ride with the head)
        assert counts[short] > 1
        caps = [n + 2 for n in counts]; caps[short] = counts[short] - 1
        out = C.run(P, of(ctxs, B), B, call, where, caps=caps)
        want_status = [0] * B.nctx; want_status[short] = P.ERR_CAPACITY
        assert out["rc"] == P.ERR_CAPACITY and out["status"].tolist() == want_status
        got, want = out["frames"][short], C.reference(P, B, short, call)
        assert got["n_out"] == counts[short] and got["res"].as_dict() == want[-1].as_dict() and (got["rows"] == C.PREFILL).all()      # count and result written, no row
        if call == "components":
            assert np.array_equal(got["image"][:B.n], C.words(want[1]))      # (the lone call's rule: the image is written)
        for i in range(B.nctx):
            if i != short:
                C.assert_frame(P, call, out["frames"][i], C.reference(P, B, i, call), "frame %d beside a short one" % i)
    # no rows asked for at all: counts and results only
    out = C.run(P, of(ctxs, B), B, call, where, want_rows=False)
    C.assert_batch(P, B, call, out, "no rows", want_rows=False)


@pytest.mark.parametrize("where", ["host", "device"])
def test_contacts_overflow_reruns_the_frames_that_need_it(P, ctxs, monkeypatch, where):
    monkeypatch.setenv("F3DS_RGC_FIRST_CAP", "64")
    B = C.batch(P, "four")
    assert C.row_count(P, B, 2, "contacts") == 0 and min(C.row_count(P, B, i, "contacts") for i in (0, 1, 3)) > 0      # (scene 2 has no contact)
    out = C.run(P, of(ctxs, B), B, "contacts", where)
    C.assert_batch(P, B, "contacts", out, "first cap 64")
    shapes = [c.launch_shape()[2] for c in of(ctxs, B)]
    assert shapes[2] == B.nctx and 1 in shapes      # (frame 2 fitted and ran with the batch only; a rerun is a launch of one frame)


# ---- 3. refusals of the call as a whole ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("call", C.CALLS)
def test_whole_call_refusals_write_nothing(P, ctxs, call):
    B = C.batch(P, "four")
    cs = of(ctxs, B)
    vp = ctypes.c_void_p
    hs = lambda ptrs: (vp * B.nctx)(*ptrs)
    h = [c.handle.value for c in cs]

    def refused(code, **kw):
        out = C.run(P, cs, B, call, "host", **kw)
        assert out["rc"] == code, (kw, out["rc"])
        assert (out["status"] == UNSET).all() and all(C.untouched(P, call, fr) for fr in out["frames"]), kw

    refused(P.ERR_ARG, handles=hs([h[0], None, h[2], h[3]]))
    refused(P.ERR_ARG, handles=hs([h[0], h[1], h[0], h[3]]))
    refused(P.ERR_UNSUPPORTED, n_regions=[B.frames[0]["K"], 0x01000000, 1, B.frames[3]["K"]], caps=[4] * 4)
    for fields in (dict(width=0), dict(depth_type=7), dict(fx=0.0), dict(depth_scale=0.0), dict(depth_pitch=3)):
        f = B.fmt.copy()
        for k, v in fields.items():
            setattr(f, k, v)
        refused(P.ERR_ARG, fmt=f, caps=[4] * 4)
    if call in ("table", "shapes", "boxes"):
        refused(P.ERR_ARG, null_rows_at=2)      # (n_regions[2] = 1 > 0)
    if call == "boxes":
        refused(P.ERR_ARG, plane_tol=-0.5)
        refused(P.ERR_ARG, plane_tol=float("nan"))
    if call == "contacts":
        refused(P.ERR_ARG, depth_tol=-0.01)
    if call == "components":
        refused(P.ERR_ARG, depth_tol=-0.01)
        refused(P.ERR_ARG, comp_is_labels_at=3)
    # nctx = 0
    lib = cs[0].lib
    st = np.full(4, UNSET, np.int32)
    z = (vp * 4)()
    nr = (ctypes.c_uint32 * 4)(1, 1, 1, 1)
    n_out = (ctypes.c_size_t * 4)(UNSET, UNSET, UNSET, UNSET)
    args = dict(table=(z, z, z, nr, 0, z, 0, None), shapes=(z, z, nr, 0, z, 0, None), boxes=(z, z, nr, 0.01, 0, z, None, 0, None), contacts=(z, z, nr, 0.05, 0, z, n_out, 0, n_out, None),
                components=(z, z, nr, None, 0, z, z, n_out, 0, n_out, None))[call]
    fn = getattr(lib, "f3ds_region_%s_batch" % call)
    for nctx in (0, -1):
        assert fn(hs(h), nctx, ctypes.byref(B.fmt), *args, st.ctypes.data) == P.ERR_ARG
    assert (st == UNSET).all()
    # and the contexts still answer
    C.assert_batch(P, B, call, C.run(P, cs, B, call, "host"), "after the refusals")


# ---- 4. lone and batch calls on the same contexts ------------------------------------------------------------------------------------------------------------------

def lone(P, ctx, B, i, call):
    fr = B.frames[i]
    a = (fr["depth"], fr["labels"], fr["K"], B.fmt)
    if call == "boxes":
        return ctx.region_boxes(*a, shapes_out=True)
    return getattr(ctx, "region_" + call)(*a)


def same_as_reference(P, B, i, call, got):
    want = C.reference(P, B, i, call)[1:]
    return len(got) == len(want) and all(g.tobytes() == w.tobytes() if isinstance(w, np.ndarray) else g.as_dict() == w.as_dict() for g, w in zip(got, want))


def test_lone_and_batch_calls_interleaved(P, ctxs):
    B, B5 = C.batch(P, "four"), C.batch(P, "five")
    cs = of(ctxs, B)
    for where in ("host", "device"):
        C.assert_batch(P, B, "boxes", C.run(P, cs, B, "boxes", where), "boxes first")
        C.assert_batch(P, B, "shapes", C.run(P, cs, B, "shapes", where), "shapes after boxes")      # (pass one of the boxes adds into the shapes' accumulators)
        C.assert_batch(P, B, "boxes", C.run(P, cs, B, "boxes", where, want_shapes=False), "boxes after shapes", want_shapes=False)
        for i in (3, 1):      # lone calls between two batches, on contexts of the batch, the large frame last
            for call in ("shapes", "boxes", "contacts", "components", "table"):
                assert same_as_reference(P, B, i, call, lone(P, cs[i], B, i, call)), (call, i)
        C.assert_batch(P, B5, "components", C.run(P, of(ctxs, B5), B5, "components", where), "another size, five contexts")
        for call in C.CALLS:
            C.assert_batch(P, B, call, C.run(P, cs, B, call, where), "after the lone calls")
        # the batch in another order of contexts: the owner of the staging changes
        rev = cs[::-1]
        C.assert_batch(P, B, "contacts", C.run(P, rev, B, "contacts", where), "contexts reversed")
        assert same_as_reference(P, B, 0, "contacts", lone(P, cs[0], B, 0, "contacts"))


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------------------------------------

def same(a, b):
    if isinstance(a, dict):
        a, b = [a[k] for k in sorted(a)], [b[k] for k in sorted(a)]
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_the_five_batch_calls_behind_segment_rgbd_batch(P):
    import torch
    k, w, h = 3, 160, 120
    imgs = [frame_images(P, 7 + i, w, h) for i in range(k)]
    fmt = imgs[0][0]
    prm = P.launch_params(voxel_res=0.02, seed_res=0.2)
    cs, others = [P.Context(0) for _ in range(k)], [P.Context(0) for _ in range(k)]
    try:
        depths, colors = [d for _, d, _c in imgs], [c for _, _d, c in imgs]
        labs = P.segment_rgbd_batch(cs, depths, colors, fmt, prm)
        assert all(np.array_equal(x, y) for x, y in zip(P.segment_rgbd_batch(others, depths, colors, fmt, prm), labs))
        nreg = [int(c.result.n_regions) for c in cs]
        assert min(nreg) > 10
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
        dd, dc, dl = [put(d) for d in depths], [put(c) for c in colors], [put(x) for x in labs]
        n = w * h
        comp = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(k)]
        crow = [torch.zeros(3 * n, dtype=torch.int32, device="cuda") for _ in range(k)]
        torch.cuda.synchronize()
        frames, status = P.region_components_batch(cs, dd, dl, nreg, fmt, rows_out=[(r, n) for r in crow], comp_out=comp, on_device=True)
        torch.cuda.synchronize()
        assert (status == 0).all()
        ncomp = [int(f[2].n_components) for f in frames]
        lone_c = [others[i].region_components(depths[i], labs[i], nreg[i], fmt) for i in range(k)]
        for i in range(k):
            assert ncomp[i] == lone_c[i][2].n_components > 10 and comp[i].cpu().numpy().view(np.uint32).tobytes() == lone_c[i][0].tobytes()
            assert crow[i].cpu().numpy().view(np.uint32)[:3 * ncomp[i]].tobytes() == lone_c[i][1].tobytes() and frames[i][2].as_dict() == lone_c[i][2].as_dict()
        images = [x[0] for x in lone_c]
        word = lambda t, count: t.cpu().numpy().view(np.uint32)[:count]
        for name, rw, kw, lone_kw in (("table", 18, dict(colors=dc), None), ("shapes", 21, {}, None), ("boxes", 24, dict(shapes_out=None), None)):
            rows = [torch.zeros(max(rw * x, 1), dtype=torch.int32, device="cuda") for x in ncomp]
            torch.cuda.synchronize()
            frames, status = getattr(P, "region_%s_batch" % name)(cs, dd, comp, ncomp, fmt, rows_out=rows, on_device=True, **kw)
            torch.cuda.synchronize()
            assert (status == 0).all()
            for i in range(k):
                want = getattr(others[i], "region_" + name)(depths[i], images[i], ncomp[i], fmt, **(dict(color=colors[i]) if name == "table" else {}))
                assert word(rows[i], rw * ncomp[i]).tobytes() == want[0].tobytes() and frames[i][-1].as_dict() == want[-1].as_dict(), (name, i)
        rb, cap = P.REGION_CONTACT_DTYPE.itemsize // 4, 20000
        trow = [torch.zeros(rb * cap, dtype=torch.int32, device="cuda") for _ in range(k)]
        torch.cuda.synchronize()
        frames, status = P.region_contacts_batch(cs, dd, comp, ncomp, fmt, rows_out=[(r, cap) for r in trow], on_device=True)
        torch.cuda.synchronize()
        assert (status == 0).all()
        for i in range(k):
            want = others[i].region_contacts(depths[i], images[i], ncomp[i], fmt)
            assert frames[i][1].as_dict() == want[1].as_dict() and word(trow[i], rb * len(want[0])).tobytes() == want[0].tobytes()
        # `others` made lone region calls only, after the same segmentation; a context that made none answers the same as both
        fresh = [P.Context(0) for _ in range(k)]
        try:
            P.segment_rgbd_batch(fresh, depths, colors, fmt, prm)
            for a, b in zip(cs, fresh):
                assert same(a.regions(), b.regions()) and same(a.voxel_cloud(), b.voxel_cloud())
                assert np.array_equal(a.recluster(prm), b.recluster(prm)) and a.result.n_regions == b.result.n_regions
        finally:
            for c in fresh:
                c.close()
    finally:
        for c in cs + others:
            c.close()
