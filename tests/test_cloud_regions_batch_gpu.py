"""f3ds_cloud_regions_batch (include/f3ds.h): three frames of different point counts in one call -- 6000 points under K = 5, 6000 points under K = 300 scattered,
and a frame of no points with K = 0 -- host and device buffers, with and without boxes, on the walk the host chooses for the batch (ordered: one frame's K
asks for it), on both forced walks and at F3DS_GRID_CAP = 1 and 3.  Each frame equals its lone call and the host function, word for word; a frame with a
bad label fails alone with its status, the call returns the status of the lowest failing frame and the other frames' outputs are the lone calls' bits;
whole-call refusals write nothing, `status` included."""
import ctypes

import numpy as np
import pytest

import cloud_regions_common as C
import region_boxes_common as B
from region_table_common import NO
from test_cloud_regions_gpu import PREFILL, SEVENS, gpu_cloud, switches, to_device

pytestmark = pytest.mark.gpu
UNSET = 777


def frames():
    """[(pts, labels, K)]: K = 5 (its labels in runs: an organised cloud), K = 300 scattered, and nothing at all"""
    a = C.patches(6000, 5, 501, scatter=False)
    b = C.patches(5000, 300, 502)
    return [(a[0], a[1], 5), (b[0], b[1], 300), (np.zeros((0, 4), np.float32), np.zeros(0, np.uint32), 0)]


@pytest.fixture(scope="module")
def ctxs(P):
    made = [P.Context(0) for _ in range(3)]
    yield made
    for c in made:
        c.close()


def run(P, ctxs, fr, where="host", boxes=True, prm=None, nctx=None):
    """the C entry point on raw buffers: (rc, [rows], [boxes], results, status); outputs prefilled with 0x5A5A5A5A words, status with 777, results with sevens"""
    k = len(fr) if nctx is None else nctx
    vp = ctypes.c_void_p
    spare = np.zeros(24, np.float32)
    rows = [np.full(32 * K, PREFILL, np.uint32) for _, _, K in fr]
    brows = [np.full(24 * K, PREFILL, np.uint32) for _, _, K in fr]
    results = (P.CloudRegionsResult * len(fr))(*[P.CloudRegionsResult(7, 7, 7, 7, 7) for _ in fr])
    status = np.full(len(fr), UNSET, np.int32)
    cnt = (ctypes.c_size_t * len(fr))(*[len(l) for _, l, _ in fr])
    nr = (ctypes.c_uint32 * len(fr))(*[K for _, _, K in fr])
    handles = (vp * len(fr))(*[c.handle for c in ctxs[:len(fr)]])
    keep = []
    if where == "device":
        import torch
        for p, l, K in fr:
            keep.append((to_device(p if len(l) else spare.reshape(-1, 4)[:1]), to_device((l if len(l) else np.zeros(1, np.uint32)).view(np.int32)),
                         to_device(np.full(max(32 * K, 1), PREFILL, np.uint32).view(np.int32)), to_device(np.full(max(24 * K, 1), PREFILL, np.uint32).view(np.int32))))
        pp, lp = (vp * len(fr))(*[x[0].data_ptr() for x in keep]), (vp * len(fr))(*[x[1].data_ptr() for x in keep])
        rp, bp = (vp * len(fr))(*[x[2].data_ptr() for x in keep]), (vp * len(fr))(*[x[3].data_ptr() for x in keep])
    else:
        pp = (vp * len(fr))(*[p.ctypes.data if len(l) else spare.ctypes.data for p, l, _ in fr]); lp = (vp * len(fr))(*[l.ctypes.data if len(l) else spare.ctypes.data for _, l, _ in fr])
        rp = (vp * len(fr))(*[r.ctypes.data if len(r) else None for r in rows]); bp = (vp * len(fr))(*[b.ctypes.data if len(b) else spare.ctypes.data for b in brows])
    on = 1 if where == "device" else 0
    rc = ctxs[0].lib.f3ds_cloud_regions_batch(handles, k, pp, cnt, lp, nr, ctypes.byref(prm) if prm is not None else None, on, rp, bp if boxes else None, on, results, status.ctypes.data)
    if where == "device":
        import torch
        torch.cuda.synchronize()
        rows = [x[2].cpu().numpy().view(np.uint32)[:32 * K].copy() for x, (_, _, K) in zip(keep, fr)]
        brows = [x[3].cpu().numpy().view(np.uint32)[:24 * K].copy() for x, (_, _, K) in zip(keep, fr)]
    return rc, [r.view(P.CLOUD_REGION_DTYPE) for r in rows], [b.view(P.REGION_BOX_DTYPE) for b in brows], results, status


_want = {}


def wanted(P, fr):
    """the host function on every frame, once"""
    if "host" not in _want:
        out = []
        for p, l, K in fr:
            rc, rows, boxes, res = C.c_cloud(P, p, l, K)
            assert rc == 0
            out.append((rows, boxes, res.as_dict()))
        _want["host"] = out
    return _want["host"]


@pytest.mark.parametrize("cap", [0, 1, 3])
@pytest.mark.parametrize("path", [None, "direct", "ordered"])
def test_each_frame_equals_its_lone_call_and_the_host_function(P, ctxs, monkeypatch, path, cap):
    switches(monkeypatch, path, cap)
    fr = frames()
    want = wanted(P, fr)
    for where in ("host", "device"):
        for boxes in (True, False):
            rc, rows, brows, results, status = run(P, ctxs, fr, where, boxes)
            assert rc == 0 and status.tolist() == [0, 0, 0]
            for i, (p, l, K) in enumerate(fr):
                C.assert_rows_equal(rows[i], want[i][0], "frame %d %s" % (i, where))
                assert results[i].as_dict() == (want[i][2] if boxes else dict(want[i][2], n_inliers=0))
                if boxes:
                    B.assert_rows_equal(P, brows[i], want[i][1], "frame %d %s boxes" % (i, where))
                else:
                    assert (brows[i].view(np.uint32) == PREFILL).all()
                lrc, lrows, lboxes, lres = gpu_cloud(P, ctxs[i], p, l, K, where, boxes="yes" if boxes else "no")      # the lone call on the same context
                assert lrc == 0 and lres.as_dict() == results[i].as_dict()
                C.assert_rows_equal(lrows, rows[i])
                assert np.array_equal(lboxes.view(np.uint32), brows[i].view(np.uint32))
            assert ctxs[0].launch_shape()[2] == 1      # (the lone calls came last)
    # which walk the batch took: one for all its frames, ordered as soon as one K asks for it
    run(P, ctxs, fr)
    assert [c.cloud_path() for c in ctxs] == [path or "ordered"] * 3 and ctxs[0].launch_shape()[2] == 3
    run(P, ctxs, [fr[0], fr[2]])
    assert [c.cloud_path() for c in ctxs[:2]] == [path or "direct"] * 2


def test_a_bad_label_fails_its_frame_alone(P, ctxs, monkeypatch):
    """A frame can fail in one way only once pixels are looked at (a label out of range, ERR_ARG), so "the status of the lowest failing frame" cannot differ
    in value from that of any failing frame: what is checked is that the call fails iff a frame does, that exactly the bad frames carry the code, and that
    the others hold the lone calls' bits."""
    switches(monkeypatch, None, 0)
    fr = frames()
    want = wanted(P, fr)
    for where in ("host", "device"):
        for bad in ([1], [0, 1]):
            g = [(p, l.copy(), K) for p, l, K in fr]
            for i in bad:
                g[i][1][-1] = g[i][2] + i      # K, or K + 1
            rc, rows, brows, results, status = run(P, ctxs, g, where)
            assert rc == P.ERR_ARG and status.tolist() == [P.ERR_ARG if i in bad else 0 for i in range(3)]
            for i in range(3):
                if i in bad:
                    assert (rows[i].view(np.uint32) == PREFILL).all() and (brows[i].view(np.uint32) == PREFILL).all() and results[i].as_dict() == SEVENS
                else:
                    C.assert_rows_equal(rows[i], want[i][0]); B.assert_rows_equal(P, brows[i], want[i][1]); assert results[i].as_dict() == want[i][2]


def test_whole_call_refusals_write_nothing(P, ctxs, monkeypatch):
    switches(monkeypatch, None, 0)
    fr = frames()

    def refused(rc, rows, brows, results, status, code):
        assert rc == code and (status == UNSET).all() and all(r.as_dict() == SEVENS for r in results)
        assert all((r.view(np.uint32) == PREFILL).all() for r in rows) and all((b.view(np.uint32) == PREFILL).all() for b in brows)
    refused(*run(P, ctxs, fr, prm=P.CloudParams(-1.0, 0)), P.ERR_ARG)
    refused(*run(P, ctxs, fr, prm=P.CloudParams(float("nan"), 0)), P.ERR_ARG)
    refused(*run(P, ctxs, fr, nctx=0), P.ERR_ARG)
    refused(*run(P, [ctxs[0], ctxs[0], ctxs[2]], fr), P.ERR_ARG)                                    # a context twice
    lib, vp = ctxs[0].lib, ctypes.c_void_p
    # NULL arrays, a NULL labels entry, too many regions in one frame: by hand, with outputs that must stay as they are
    k = 3
    handles = (vp * k)(*[c.handle for c in ctxs])
    cnt = (ctypes.c_size_t * k)(*[len(l) for _, l, _ in fr]); nr = (ctypes.c_uint32 * k)(*[K for _, _, K in fr])
    spare = np.zeros(24, np.float32)
    pp = (vp * k)(*[p.ctypes.data if len(l) else spare.ctypes.data for p, l, _ in fr]); lp = (vp * k)(*[l.ctypes.data if len(l) else spare.ctypes.data for _, l, _ in fr])
    rows = [np.full(32 * K, PREFILL, np.uint32) for _, _, K in fr]
    rp = (vp * k)(*[r.ctypes.data if len(r) else None for r in rows])
    status = np.full(k, UNSET, np.int32)
    results = (P.CloudRegionsResult * k)(*[P.CloudRegionsResult(7, 7, 7, 7, 7) for _ in fr])
    good = [handles, k, pp, cnt, lp, nr, None, 0, rp, None, 0, results, status.ctypes.data]
    for at in (0, 2, 3, 4, 5, 8):
        a = list(good); a[at] = None
        assert lib.f3ds_cloud_regions_batch(*a) == P.ERR_ARG, at
    lp2 = (vp * k)(lp[0], None, lp[2])
    a = list(good); a[4] = lp2
    assert lib.f3ds_cloud_regions_batch(*a) == P.ERR_ARG
    nr2 = (ctypes.c_uint32 * k)(5, 0x01000000, 0)
    a = list(good); a[5] = nr2
    assert lib.f3ds_cloud_regions_batch(*a) == P.ERR_UNSUPPORTED
    bp = (vp * k)(spare.ctypes.data, None, spare.ctypes.data)                                      # boxes for every frame or for none
    a = list(good); a[9] = bp
    assert lib.f3ds_cloud_regions_batch(*a) == P.ERR_ARG
    assert (status == UNSET).all() and all(r.as_dict() == SEVENS for r in results) and all((r == PREFILL).all() for r in rows)
    assert lib.f3ds_cloud_regions_batch(*good) == 0 and status.tolist() == [0, 0, 0]


def test_package_function(P, ctxs, monkeypatch):
    switches(monkeypatch, None, 0)
    fr = frames()
    want = wanted(P, fr)
    out, status = P.cloud_regions_batch(ctxs, [p for p, _, _ in fr], [l for _, l, _ in fr], [K for _, _, K in fr], boxes_out=True)
    assert status.tolist() == [0, 0, 0]
    for i, (rows, boxes, res) in enumerate(out):
        C.assert_rows_equal(rows, want[i][0]); B.assert_rows_equal(P, boxes, want[i][1]); assert res.as_dict() == want[i][2]
    out, status = P.cloud_regions_batch(ctxs, [p for p, _, _ in fr], [l for _, l, _ in fr], [K for _, _, K in fr])
    assert status.tolist() == [0, 0, 0] and all(len(o) == 2 for o in out)
    C.assert_rows_equal(out[1][0], want[1][0])
    lab = fr[1][1].copy(); lab[0] = 300
    out, status = P.cloud_regions_batch(ctxs, [p for p, _, _ in fr], [fr[0][1], lab, fr[2][1]], [K for _, _, K in fr])
    assert status.tolist() == [0, P.ERR_ARG, 0] and out[1] == (None, None)
    with pytest.raises(P.F3dsError):
        P.cloud_regions_batch(ctxs, [p for p, _, _ in fr], [l for _, l, _ in fr], [K for _, _, K in fr], params=P.CloudParams(-1.0, 0))
