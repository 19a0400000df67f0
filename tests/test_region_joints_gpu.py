"""The region joints on the device (f3ds_region_joints: the shapes' kernels, d_pair_init, d_joint_accum, the record sort, d_joint_finish: JointRule of
csrc/f3ds_joints.inc over the pair skeleton of csrc/f3ds_pairs.inc) against f3ds_region_joints_host, bit for bit.  The frames are the smallest at which the kernels can go wrong: 300 x 7 and 257 x 5 are
wider than a workgroup (spans straddle rows; at 300 x 7 the accumulate launch has two workgroups, so a pair's two pixels lie in different spans), 64 x 48 are
the analytic scenes, 33 x 31 with every pixel its own region has some 1400 pairs in one span: eleven times the 128 slots of the LDS table, so pairs become
records of their own.  The rerun with room for all records (F3DS_RGJ_FIRST_CAP = 16) and the narrow launches (F3DS_GRID_CAP = 1, 3, 8) run in fresh child
processes; 96 x 96 single-pixel regions have more rows than the 2048 of the first download."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import region_joints_common as J
import region_shapes_common as S
from conftest import ROOT
from region_joints_common import PREFILL
from rgbd_common import frame_images

pytestmark = pytest.mark.gpu
LDS_SLOTS, FIRST_ROWS, SHORT_FIRST_CAP = 128, 2048, 16      # RGJ_SLOTS and RGJ_FIRST_ROWS of csrc/f3ds_joints.inc; the short first record buffer of the rerun
SEVENS = dict(n_regions=7, n_joints=7, n_surface=7, reserved=7, n_pairs=7, n_close=7)


# ---- 1. small frames, every buffer location ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("want_shapes", [True, False])
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("case", J.SMALL_FRAMES, ids=lambda c: "%s-%dx%d-%s" % c)
def test_small_frame_equals_the_host_function(P, gpu_ctx, case, where, want_shapes):
    sc = J.small_frame(P, case)
    rows, res = J.check_device(P, gpu_ctx, sc, case, where, "tight", want_shapes)
    if case[0] in J.ANALYTIC:
        assert len(rows) == 1 and int(rows["kind"][0]) & 0xFF == J.ANALYTIC[case[0]]
    if case[0] == "own":
        assert len(rows) > 10 * LDS_SLOTS and 0 < res["n_surface"] < len(rows)
    if case[0] == "steps":
        assert ((rows["n_close"] > 0) & (rows["n_close"] < rows["n_pairs"])).any()


@pytest.mark.parametrize("where", ["host", "device"])
def test_padded_rows_and_other_parameters(P, gpu_ctx, where):
    sc = J.small_frame(P, ("steps", 300, 7, "f32"))
    for prm in ((0.0, 0.01, 0.9659258), (1.0e30, 0.0, 1.0), (0.05, float("inf"), -1.0)):
        J.check_device(P, gpu_ctx, sc, "steps-300x7", where, "padded", True, prm)
    sc = J.small_frame(P, ("blocks", 300, 7, "u16"))
    J.check_device(P, gpu_ctx, sc, ("blocks", 300, 7, "u16"), where, "padded", True)


@pytest.mark.parametrize("where", ["host", "device"])
def test_more_rows_than_the_first_download(P, gpu_ctx, where):
    sc = J.own_region_scene(P, 96, 96)
    rows, res = J.check_device(P, gpu_ctx, sc, "own-96x96", where, "tight", where == "host")
    assert len(rows) == 2 * 96 * 95 > FIRST_ROWS and res["n_surface"] == len(rows)


@pytest.mark.parametrize("where", ["host", "device"])
def test_count_only_and_capacity(P, gpu_ctx, where):
    case = ("blocks", 300, 7, "u16")
    sc = J.small_frame(P, case)
    wrows, wshapes, wres = J.host_joints(P, case, sc)
    n = len(wrows)
    assert n > 2
    rc, rows, n_out, shapes, res = J.gpu_joints(P, gpu_ctx, sc, None, where, cap=n + 5, count_only=True)
    assert rc == 0 and n_out == n and res.as_dict() == wres and (rows.view(np.uint32) == PREFILL).all()
    S.assert_rows_equal(P, shapes, wshapes)
    rc, rows, n_out, shapes, res = J.gpu_joints(P, gpu_ctx, sc, None, where, cap=n - 1)
    assert rc == P.ERR_CAPACITY and n_out == n and res.as_dict() == wres and (rows.view(np.uint32) == PREFILL).all()
    S.assert_rows_equal(P, shapes, wshapes)
    rc, rows, n_out, shapes, res = J.gpu_joints(P, gpu_ctx, sc, None, where, cap=n)
    assert rc == 0 and n_out == n
    J.assert_rows_equal(rows, wrows)


# ---- 2. the rerun and the narrow launches: fresh child processes --------------------------------------------------------------------------------------------

def run_child(env, cap):
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import conftest, region_joints_common as J\n"
            "print(json.dumps(J.child_run(conftest.pkg(), %d)))\n") % (ROOT, os.path.join(ROOT, "tests"), cap)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, F3DS_DEV="1", **env))
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_rerun_with_room_for_all_records(P):
    got = run_child(dict(F3DS_RGJ_FIRST_CAP=str(SHORT_FIRST_CAP)), 0)
    assert len(got) == len(J.SMALL_FRAMES)
    want = {"%s-%dx%d" % c[:3]: len(J.host_joints(P, c, J.small_frame(P, c))[0]) for c in J.SMALL_FRAMES}
    assert {k: v[0] for k, v in got.items()} == want
    assert want["own-33x31"] > SHORT_FIRST_CAP and want["blocks-97x61"] > SHORT_FIRST_CAP      # more rows than records the first run had room for: those frames ran twice


@pytest.mark.parametrize("cap", [1, 3, 8])
def test_narrow_launches(P, cap):
    got = run_child(dict(F3DS_GRID_CAP=str(cap)), cap)
    assert len(got) == len(J.SMALL_FRAMES) and got["own-33x31"][0] > 10 * LDS_SLOTS


# ---- 3. errors ----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["host", "device"])
def test_a_bad_label_is_found_on_the_device_and_leaves_everything(P, gpu_ctx, where):
    case = ("blocks", 300, 7, "u16")
    sc = J.small_frame(P, case)
    K = sc["n_regions"]
    for at, value, invalid_depth in ((-1, K, False), (0, K + 5, False), (-1, 0xFFFFFFFE, True)):
        lab = sc["labels"].copy(); lab.reshape(-1)[at] = value
        depth = sc["depth"].copy()
        if invalid_depth:
            depth.reshape(-1)[at] = 0
        rc, rows, n_out, shapes, res = J.gpu_joints(P, gpu_ctx, dict(sc, labels=lab, depth=depth), None, where)
        assert rc == P.ERR_ARG
        assert (rows.view(np.uint32) == PREFILL).all() and (shapes.view(np.uint32) == PREFILL).all() and n_out == 777 and res.as_dict() == SEVENS
    J.check_device(P, gpu_ctx, sc, case, where)      # and the context still answers


def test_argument_errors(P, gpu_ctx):
    lib = gpu_ctx.lib
    sc = J.scene(P, 1, 3, 2, "u16")
    fmt, K = sc["fmt"], sc["n_regions"]
    d, l = sc["depth"], sc["labels"]
    rows = np.full(20 * 16, PREFILL, np.uint32)
    shapes = np.full(21 * K, PREFILL, np.uint32)
    n_out = ctypes.c_size_t(777)
    res = P.RegionJointsResult(7, 7, 7, 7, 7, 7)
    prm = J.params_of(P, J.DEFAULTS)
    for on_dev in (0, 1):      # (every one of these is refused before a buffer is looked at: host pointers do for both forms)
        good = [gpu_ctx.handle, ctypes.byref(fmt), d.ctypes.data, l.ctypes.data, K, ctypes.byref(prm), on_dev, rows.ctypes.data, 16, shapes.ctypes.data, on_dev, ctypes.byref(n_out),
                ctypes.byref(res)]

        def refused(args, code, why):
            assert lib.f3ds_region_joints(*args) == code, why
            assert (rows == PREFILL).all() and (shapes == PREFILL).all() and n_out.value == 777 and res.as_dict() == SEVENS, why

        for k in (0, 1, 2, 3, 11):
            a = list(good); a[k] = None
            refused(a, P.ERR_ARG, k)
        for fields in (dict(width=0), dict(depth_type=7), dict(fx=0.0), dict(fy=float("nan")), dict(depth_scale=0.0), dict(cx=float("inf")), dict(depth_pitch=3)):
            f = fmt.copy()
            for k, v in fields.items():
                setattr(f, k, v)
            a = list(good); a[1] = ctypes.byref(f)
            refused(a, P.ERR_ARG, fields)
        for bad in ((-0.01, 0.01, 0.9), (float("nan"), 0.01, 0.9), (float("inf"), 0.01, 0.9), (0.05, -0.5, 0.9), (0.05, float("nan"), 0.9), (0.05, 0.01, float("nan")),
                    (0.05, 0.01, 1.5)):
            p = J.params_of(P, bad)
            a = list(good); a[5] = ctypes.byref(p)
            refused(a, P.ERR_ARG, bad)
        a = list(good); a[4] = 0x01000000
        refused(a, P.ERR_UNSUPPORTED, "regions")
        f = fmt.copy(); f.width = 0x8000; f.height = 0x4000
        a = list(good); a[1] = ctypes.byref(f)
        refused(a, P.ERR_UNSUPPORTED, "pixels")
    # NULL params are the defaults; zero rows: no region, one region, no labelled pixel
    rc, got, n, _, r = J.gpu_joints(P, gpu_ctx, sc)
    want = J.host_joints(P, "3x2", sc)
    assert rc == 0 and n == len(want[0]) and r.as_dict() == want[2]
    a = [gpu_ctx.handle, ctypes.byref(fmt), d.ctypes.data, l.ctypes.data, K, None, 0, rows.ctypes.data, 16, None, 0, ctypes.byref(n_out), None]
    assert lib.f3ds_region_joints(*a) == 0 and n_out.value == n
    J.assert_rows_equal(rows.view(P.REGION_JOINT_DTYPE)[:n], want[0])
    none = np.full((2, 3), 0xFFFFFFFF, np.uint32)
    rc, got, n, _, r = J.gpu_joints(P, gpu_ctx, dict(sc, labels=none, n_regions=0))
    assert rc == 0 and n == 0 and r.as_dict() == dict(n_regions=0, n_joints=0, n_surface=0, reserved=0, n_pairs=0, n_close=0)
    assert J.gpu_joints(P, gpu_ctx, dict(sc, n_regions=0))[0] == P.ERR_ARG      # label 0 >= 0 regions
    rc, got, n, sh, r = J.gpu_joints(P, gpu_ctx, dict(sc, labels=np.zeros((2, 3), np.uint32), n_regions=1))
    assert rc == 0 and n == 0 and r.as_dict() == dict(n_regions=1, n_joints=0, n_surface=0, reserved=0, n_pairs=0, n_close=0) and sh["n_pixels"][0] > 0
    rc, got, n, sh, r = J.gpu_joints(P, gpu_ctx, dict(sc, depth=np.zeros((2, 3), np.uint16)))
    assert rc == 0 and n == 0 and r.as_dict() == dict(n_regions=K, n_joints=0, n_surface=0, reserved=0, n_pairs=0, n_close=0) and (sh["n_pixels"] == 0).all()


# ---- 4. the package, lone and batch -------------------------------------------------------------------------------------------------------------------------

def to_device(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
    torch.cuda.synchronize()
    return t


def test_package_method(P, gpu_ctx):
    case = ("blocks", 300, 7, "u16")
    sc = J.small_frame(P, case)
    K = sc["n_regions"]
    wrows, wshapes, wres = J.host_joints(P, case, sc)
    rows, res = gpu_ctx.region_joints(sc["depth"], sc["labels"], K, sc["fmt"])
    J.assert_rows_equal(rows, wrows)
    assert res.as_dict() == wres and rows.dtype == P.REGION_JOINT_DTYPE
    out = np.zeros(len(wrows) + 3, P.REGION_JOINT_DTYPE)
    got, shapes, _ = gpu_ctx.region_joints(sc["depth"], sc["labels"], K, sc["fmt"], params=P.default_joint_params(), rows_out=out, shapes_out=True)
    assert got.base is out and len(got) == len(wrows)
    J.assert_rows_equal(got, wrows)
    S.assert_rows_equal(P, shapes, wshapes)
    with pytest.raises(P.F3dsError):
        gpu_ctx.region_joints(sc["depth"], sc["labels"], K, sc["fmt"], rows_out=np.zeros(2, P.REGION_JOINT_DTYPE))
    # device pointers through the package
    import torch
    dd, dl = to_device(sc["depth"].view(np.uint8)), to_device(sc["labels"].view(np.int32))
    cap = len(wrows) + 1
    dr, ds = torch.zeros(20 * cap, dtype=torch.int32, device="cuda"), torch.zeros(21 * K, dtype=torch.int32, device="cuda")
    none, none2, res4 = gpu_ctx.region_joints(dd.data_ptr(), dl.data_ptr(), K, sc["fmt"], rows_out=(dr.data_ptr(), cap), shapes_out=ds.data_ptr(), on_device=True)
    torch.cuda.synchronize()
    assert none is None and none2 is None and res4.as_dict() == wres
    J.assert_rows_equal(dr.cpu().numpy().view(P.REGION_JOINT_DTYPE)[:len(wrows)], wrows)
    S.assert_rows_equal(P, ds.cpu().numpy().view(P.REGION_SHAPE_DTYPE), wshapes)
    assert gpu_ctx.region_joints(dd.data_ptr(), dl.data_ptr(), K, sc["fmt"], on_device=True)[1].as_dict() == wres      # count only


@pytest.fixture(scope="module")
def three(P):
    ctxs = [P.Context(0) for _ in range(3)]
    yield ctxs
    for c in ctxs:
        c.close()


def test_batch_statuses_and_bits(P, three):
    w, h = 67, 45
    s7 = J.scene(P, 7, w, h, "f32")
    fmt = s7["fmt"]
    own = J.checker_scene(P, w, h)
    frames = [s7, dict(own, fmt=fmt), dict(s7, labels=np.ascontiguousarray(s7["labels"][::-1]))]      # (one format for the batch: scene 7's, f32 metres)
    lone = [P.region_joints_host(f["depth"], f["labels"], f["n_regions"], fmt, want_shapes=True) for f in frames]
    depths, labels, K = [f["depth"] for f in frames], [f["labels"] for f in frames], [f["n_regions"] for f in frames]
    # all good: the bits of the lone host function, shapes included
    out, status = P.region_joints_batch(three, depths, labels, K, fmt, shapes_out=True)
    assert status.tolist() == [0, 0, 0]
    for (rows, shapes, res), (wrows, wshapes, wres) in zip(out, lone):
        J.assert_rows_equal(rows, wrows)
        S.assert_rows_equal(P, shapes, wshapes)
        assert res.as_dict() == wres.as_dict()
    assert len(lone[1][0]) > FIRST_ROWS      # (the second frame's rows come in a second download)
    # ... and of the lone device call on the same contexts
    for i, f in enumerate(frames):
        rows, res = three[i].region_joints(f["depth"], f["labels"], f["n_regions"], fmt)
        J.assert_rows_equal(rows, lone[i][0])
    # frame 0 with a bad label, frame 2 with a short capacity: each fails alone
    bad = labels[0].copy(); bad[3, 5] = K[0] + 1
    n2 = len(lone[2][0])
    bufs = [np.full(20 * (len(lone[0][0]) + 1), PREFILL, np.uint32).view(P.REGION_JOINT_DTYPE), np.full(20 * (len(lone[1][0]) + 1), PREFILL, np.uint32).view(P.REGION_JOINT_DTYPE),
            np.full(20 * (n2 - 1), PREFILL, np.uint32).view(P.REGION_JOINT_DTYPE)]
    out, status = P.region_joints_batch(three, depths, [bad, labels[1], labels[2]], K, fmt, rows_out=bufs)
    assert status.tolist() == [P.ERR_ARG, 0, P.ERR_CAPACITY]
    assert out[0] == (None, None) and (bufs[0].view(np.uint32) == PREFILL).all()
    J.assert_rows_equal(out[1][0], lone[1][0])
    assert out[1][1].as_dict() == lone[1][2].as_dict() and (bufs[1][len(lone[1][0]):].view(np.uint32) == PREFILL).all()
    assert out[2][0] is None and out[2][1].as_dict() == lone[2][2].as_dict() and (bufs[2].view(np.uint32) == PREFILL).all()
    # the raw call's return code is the lowest failing frame's
    vp = ctypes.c_void_p
    handles = (vp * 3)(*[c.handle for c in three])
    lab = [np.ascontiguousarray(x, np.uint32) for x in (bad, labels[1], labels[2])]
    dep = [np.ascontiguousarray(x, np.float32) for x in depths]
    dp, lp = (vp * 3)(*[x.ctypes.data for x in dep]), (vp * 3)(*[x.ctypes.data for x in lab])
    nr = (ctypes.c_uint32 * 3)(*K)
    rp, caps = (vp * 3)(*[b.ctypes.data for b in bufs]), (ctypes.c_size_t * 3)(*[len(b) for b in bufs])
    n_out, st = (ctypes.c_size_t * 3)(777, 777, 777), np.full(3, 1, np.int32)
    f = fmt.copy()
    rc = P.load_library().f3ds_region_joints_batch(handles, 3, ctypes.byref(f), dp, lp, nr, None, 0, rp, caps, None, 0, n_out, None, st.ctypes.data)
    assert rc == P.ERR_ARG and st.tolist() == [P.ERR_ARG, 0, P.ERR_CAPACITY] and list(n_out) == [777, len(lone[1][0]), n2]
    # a repeated context and a NULL entry are refused as a whole: no status, no count
    for hs in ((vp * 3)(three[0].handle, three[1].handle, three[0].handle), (vp * 3)(three[0].handle, None, three[2].handle)):
        n_out, st = (ctypes.c_size_t * 3)(777, 777, 777), np.full(3, 1, np.int32)
        for b in bufs:
            b.view(np.uint32)[:] = PREFILL
        rc = P.load_library().f3ds_region_joints_batch(hs, 3, ctypes.byref(f), dp, lp, nr, None, 0, rp, caps, None, 0, n_out, None, st.ctypes.data)
        assert rc == P.ERR_ARG and st.tolist() == [1, 1, 1] and list(n_out) == [777] * 3 and all((b.view(np.uint32) == PREFILL).all() for b in bufs)


@pytest.mark.parametrize("where", ["host", "device"])
def test_batch_overflow_reruns_the_frames_that_need_it(P, three, monkeypatch, where):
    """The rerun with room for all records inside a batch (the contacts' twin: test_region_batch_gpu.py): with room for 64 records the checker frame --
    thousands of rows, and a row needs at least one record -- runs again alone; the frame of one region has no pair, hence no record, and runs with the batch
    only."""
    monkeypatch.setenv("F3DS_RGJ_FIRST_CAP", "64")
    w, h = 67, 45
    s7 = J.scene(P, 7, w, h, "f32")
    fmt = s7["fmt"]
    frames = [s7, dict(J.checker_scene(P, w, h), fmt=fmt), dict(s7, labels=np.zeros((h, w), np.uint32), n_regions=1)]      # (one format for the batch: scene 7's, f32 metres)
    want = [P.region_joints_host(f["depth"], f["labels"], f["n_regions"], fmt, want_shapes=True) for f in frames]
    assert len(want[1][0]) > 64 and len(want[2][0]) == 0      # (by the host function alone: the checker frame cannot fit, the last one has nothing to fit)
    depths, labels, K = [f["depth"] for f in frames], [f["labels"] for f in frames], [f["n_regions"] for f in frames]
    if where == "host":
        got, status = P.region_joints_batch(three, depths, labels, K, fmt, shapes_out=True)
    else:
        import torch
        dd = [to_device(np.ascontiguousarray(d, np.float32)) for d in depths]
        dl = [to_device(np.ascontiguousarray(x, np.uint32).view(np.int32)) for x in labels]
        caps = [len(wrows) + 1 for wrows, _, _ in want]
        dr = [torch.zeros(20 * c, dtype=torch.int32, device="cuda") for c in caps]
        ds = [torch.zeros(21 * k, dtype=torch.int32, device="cuda") for k in K]
        out, status = P.region_joints_batch(three, dd, dl, K, fmt, rows_out=[(r.data_ptr(), c) for r, c in zip(dr, caps)], shapes_out=ds, on_device=True)
        torch.cuda.synchronize()
        assert all(o[0] is None and o[1] is None for o in out)
        got = [(r.cpu().numpy().view(P.REGION_JOINT_DTYPE)[:o[2].n_joints], s.cpu().numpy().view(P.REGION_SHAPE_DTYPE), o[2]) for r, s, o in zip(dr, ds, out)]
    assert status.tolist() == [0, 0, 0]
    for (rows, shapes, res), (wrows, wshapes, wres) in zip(got, want):
        J.assert_rows_equal(rows, wrows)
        S.assert_rows_equal(P, shapes, wshapes)
        assert res.as_dict() == wres.as_dict()
    assert three[2].launch_shape()[2] == 3 and three[1].launch_shape()[2] == 1      # (a rerun is a launch of one frame)


# ---- 5. end to end: the context is untouched ------------------------------------------------------------------------------------------------------------------

def same(a, b):
    """two answers of a context (a tuple or a dict of arrays), byte for byte"""
    if isinstance(a, dict):
        a, b = [a[k] for k in sorted(a)], [b[k] for k in sorted(a)]
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_the_joints_of_a_segmented_frame_and_the_context_afterwards(P):
    fmt, depth, color = frame_images(P, 7, 160, 120)
    prm = P.launch_params(voxel_res=0.02, seed_res=0.2)
    ctx, other = P.Context(0), P.Context(0)
    try:
        lab = ctx.segment_rgbd(depth, color, fmt, prm); K = int(ctx.result.n_regions)
        assert np.array_equal(other.segment_rgbd(depth, color, fmt, prm), lab) and K > 10
        rows, shapes, res = ctx.region_joints(depth, lab, K, fmt, shapes_out=True)
        wrows, wshapes, wres = P.region_joints_host(depth, lab, K, fmt, want_shapes=True)
        assert res.as_dict() == wres.as_dict() and len(rows) > 0
        J.assert_rows_equal(rows, wrows)
        S.assert_rows_equal(P, shapes, wshapes)
        # the contacts and the shapes of the same context: the same bits
        crows, _ = ctx.region_contacts(depth, lab, K, fmt)
        for k in ("a", "b", "n_pairs", "n_close"):
            assert np.array_equal(rows[k], crows[k]), k
        S.assert_rows_equal(P, ctx.region_shapes(depth, lab, K, fmt)[0], shapes)
        # the context answers as one that never made the call
        assert same(ctx.regions(), other.regions()) and same(ctx.voxel_cloud(), other.voxel_cloud())
        assert np.array_equal(ctx.recluster(prm), other.recluster(prm)) and ctx.result.n_regions == other.result.n_regions
    finally:
        ctx.close(); other.close()
