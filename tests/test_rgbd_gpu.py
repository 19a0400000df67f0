"""RGB-D frames on the device: f3ds_segment_rgbd[_batch] builds the records with d_deproject (csrc/f3ds_kernels.inc) and is defined as f3ds_segment on
f3ds_deproject's records.  The records themselves are read back (Context.points()) and compared byte for byte with the host's for every shape, format and row
layout of tests/test_rgbd_cpu.py and a wide flat frame, at the default launch width and at 1 and 3 workgroups per frame; labels, counts and every debug array
are compared with the point path's and the oracle's; the context's later calls, all-invalid frames and the frame pipeline follow."""
import ctypes

import numpy as np
import pytest

from conftest import ALL_DEBUG, first_mismatch, same_bits
from golden_cases import synthetic_truth
from rgbd_common import KINDS, LAYOUTS, SIZES, case_images, frame_images, laid_out

pytestmark = pytest.mark.gpu
RESULT_FIELDS = ("n_points", "n_finite", "n_voxels", "octree_depth", "n_seed_cells", "n_seeds", "n_supervoxels", "n_edges", "n_merges", "n_regions", "sweeps")
WIDE = (4099, 3)        # a row crosses 17 workgroups and ends 3 pixels into the last one
PARAMS = {(160, 120): dict(voxel_res=0.02, seed_res=0.2), (320, 240): dict(voxel_res=0.012, seed_res=0.1), (67, 45): dict(voxel_res=0.03, seed_res=0.3)}


def params_for(P, width, height):
    return P.launch_params(**PARAMS.get((width, height), dict(voxel_res=0.02, seed_res=0.2)))


def to_device(arr):
    """A torch tensor on the GPU holding the array's bytes (torch is the suite's way to device memory of its own)."""
    import torch
    t = torch.from_numpy(arr).cuda()
    torch.cuda.synchronize()
    return t


def assert_records(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert same_bits(got, want), (what, first_mismatch("records", want, got))
    assert np.array_equal(got[:, 3].view(np.uint32), want[:, 3].view(np.uint32)), what


def raw_segment_rgbd(P, ctx, fmt, depth_ptr, color_ptr, on_device, prm):
    """f3ds_segment_rgbd on raw pointers (host labels); returns (rc, labels)."""
    labels = np.empty(int(fmt.width) * int(fmt.height), np.uint32)
    rc = ctx.lib.f3ds_segment_rgbd(ctx.handle, ctypes.byref(fmt), ctypes.c_void_p(depth_ptr), ctypes.c_void_p(color_ptr), 1 if on_device else 0, ctypes.byref(prm),
                                   labels.ctypes.data, 0, ctypes.byref(ctx.result))
    ctx._n = len(labels)
    return rc, labels


def raw_segment(P, ctx, pts, prm):
    labels = np.empty(len(pts), np.uint32)
    rc = ctx.lib.f3ds_segment(ctx.handle, pts.ctypes.data, len(pts), 0, ctypes.byref(prm), labels.ctypes.data, 0, ctypes.byref(ctx.result))
    ctx._n = len(pts)
    return rc, labels


def same_results(a, b):
    return [f for f in RESULT_FIELDS if getattr(a, f) != getattr(b, f)]


def copy_result(P, r):
    out = P.Result()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(r), ctypes.sizeof(P.Result))
    return out


@pytest.fixture(scope="module")
def ref_ctx(P, gpu_ctx):
    """A second context, for the point-path side of every comparison (gpu_ctx runs the rgbd side)."""
    ctx = P.Context(0)
    yield ctx
    ctx.close()


class PointRuns:
    """segment(records) once per distinct (records, parameters): labels, result and, on request, the debug arrays."""

    def __init__(self, P, ctx):
        self.P, self.ctx, self.runs = P, ctx, {}

    def get(self, pts, prm, debug=False):
        key = (pts.tobytes(), bytes(ctypes.string_at(ctypes.addressof(prm), ctypes.sizeof(prm))))
        run = self.runs.get(key)
        if run is None or (debug and "debug" not in run):
            rc, labels = raw_segment(self.P, self.ctx, pts, prm)
            run = dict(rc=rc, labels=labels, result=copy_result(self.P, self.ctx.result))
            if rc == 0 and debug and self.ctx.result.n_voxels:
                run["debug"] = {w: self.ctx.debug(w) for w in ALL_DEBUG}
                run["path"] = self.ctx.stage0_path()
            self.runs[key] = run
        return run


@pytest.fixture(scope="module")
def point_runs(P, ref_ctx):
    return PointRuns(P, ref_ctx)


@pytest.fixture(scope="module")
def frames(P):
    """The u16 + RGB8 images of the frames the parity, state and stream tests use, with their records."""
    out = {}
    for (w, h), seeds in (((160, 120), (7, 8, 9, 10)), ((67, 45), (7, 8, 9, 10)), (WIDE, (7,))):
        for s in seeds:
            fmt, depth, color = frame_images(P, s, w, h)
            out[(w, h, s)] = dict(fmt=fmt, depth=depth, color=color, records=P.deproject(fmt, depth, color))
    return out


# ---- 1. the records ---------------------------------------------------------------------------------------------------------------------------------

RECORD_CASES = [(w, h, dk, ck, lay) for (w, h) in SIZES for (dk, ck) in KINDS for lay in LAYOUTS] + [WIDE + ("u16", "rgb8", lay) for lay in LAYOUTS] + \
               [WIDE + ("f32", "rgba8", "padded")]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("width,height,depth_kind,color_kind,layout", RECORD_CASES)
def test_records_equal_the_hosts(P, gpu_ctx, point_runs, width, height, depth_kind, color_kind, layout, where):
    fmt, depth, color = case_images(P, width, height, depth_kind, color_kind)
    want = P.deproject(fmt, depth, color)
    f, dbuf, cbuf = laid_out(fmt, depth, color, layout)
    prm = params_for(P, width, height)
    if where == "device":
        dd, dc = to_device(dbuf), to_device(cbuf)
        rc, labels = raw_segment_rgbd(P, gpu_ctx, f, dd.data_ptr(), dc.data_ptr(), True, prm)
    else:
        rc, labels = raw_segment_rgbd(P, gpu_ctx, f, dbuf.ctypes.data, cbuf.ctypes.data, False, prm)
    ref = point_runs.get(want, prm)
    assert rc == ref["rc"]                                      # (whatever f3ds_segment makes of a frame of one or six points, the rgbd call makes the same)
    assert_records(gpu_ctx.points(), want, (width, height, depth_kind, color_kind, layout, where))
    if rc == 0:
        assert np.array_equal(labels, ref["labels"]) and not same_results(gpu_ctx.result, ref["result"])


def test_bad_arguments_with_a_context(P, gpu_ctx, point_runs):
    fmt, depth, color = case_images(P, 3, 2, "u16", "rgb8")
    prm = params_for(P, 3, 2)
    d, c = depth.ctypes.data, color.ctypes.data
    for fields in (dict(width=0), dict(depth_type=7), dict(color_format=-2), dict(fx=0.0), dict(fy=float("nan")), dict(depth_scale=0.0), dict(cx=float("inf")),
                   dict(depth_pitch=4), dict(depth_pitch=7), dict(color_pitch=8)):
        f = fmt.copy()
        for k, v in fields.items():
            setattr(f, k, v)
        assert raw_segment_rgbd(P, gpu_ctx, f, d, c, False, prm)[0] == P.ERR_ARG, fields
    assert raw_segment_rgbd(P, gpu_ctx, fmt, 0, c, False, prm)[0] == P.ERR_ARG
    assert raw_segment_rgbd(P, gpu_ctx, fmt, d, 0, False, prm)[0] == P.ERR_ARG
    assert gpu_ctx.lib.f3ds_segment_rgbd(gpu_ctx.handle, ctypes.byref(fmt), d, c, 0, None, None, 0, None) == P.ERR_ARG
    assert raw_segment_rgbd(P, gpu_ctx, fmt, d, c, False, prm)[0] == point_runs.get(P.deproject(fmt, depth, color), prm)["rc"]      # ... and the context still works


# ---- 2. parity with the point path and the oracle ----------------------------------------------------------------------------------------------------

def assert_same_frame(ctx, labels, ref, what):
    assert not same_results(ctx.result, ref["result"]), (what, same_results(ctx.result, ref["result"]))
    problems = [m for m in (first_mismatch(w, ref["debug"][w], ctx.debug(w)) for w in ALL_DEBUG) if m]
    assert not problems, "%s:\n%s" % (what, "\n".join(problems))
    assert np.array_equal(labels, ref["labels"]), what
    a, b = ctx.result.lambda_, ref["result"].lambda_
    assert (np.isnan(a) and np.isnan(b)) or a == b, what


@pytest.mark.parametrize("width,height", [(160, 120), (67, 45)])
def test_lone_frame_equals_the_point_path_and_the_oracle(P, gpu_ctx, point_runs, frames, oracle, width, height):
    fr = frames[(width, height, 7)]
    prm = params_for(P, width, height)
    labels = gpu_ctx.segment_rgbd(fr["depth"], fr["color"], fr["fmt"], prm)
    assert gpu_ctx.stage0_path() == "sort"                      # a lone frame
    ref = point_runs.get(fr["records"], prm, debug=True)
    assert ref["rc"] == 0 and ref["path"] == "sort"
    assert_same_frame(gpu_ctx, labels, ref, (width, height))
    rc, olab, ores, oh = oracle.segment(fr["records"], prm)
    assert rc == 0
    assert np.array_equal(labels, olab)
    assert first_mismatch("MERGES", oh.get("MERGES"), gpu_ctx.debug("MERGES")) is None
    assert (ores.n_voxels, ores.n_supervoxels, ores.n_regions) == (gpu_ctx.result.n_voxels, gpu_ctx.result.n_supervoxels, gpu_ctx.result.n_regions)
    assert ores.n_regions > 10 and ores.n_supervoxels > 100    # not a degenerate frame
    oh.close()


@pytest.mark.parametrize("width,height,res", [(160, 120, (0.02, 0.2)), (67, 45, (0.03, 0.3)), (160, 120, (0.03, 0.3))])
def test_batch_of_four_equals_the_point_path(P, frames, oracle, width, height, res):
    prm = P.launch_params(voxel_res=res[0], seed_res=res[1])
    frs = [frames[(width, height, s)] for s in (7, 8, 9, 10)]
    assert len({f["records"].tobytes() for f in frs}) == 4
    a = [P.Context(0) for _ in range(4)]; b = [P.Context(0) for _ in range(4)]
    try:
        got = P.segment_rgbd_batch(a, [f["depth"] for f in frs], [f["color"] for f in frs], frs[0]["fmt"], prm)
        want = P.segment_batch(b, [f["records"] for f in frs], prm)
        paths = [c.stage0_path() for c in b]
        print("stage 0 of the batch (%d x %d, voxel_res %g): %s" % (width, height, res[0], paths))
        if res[0] == 0.03 and (width, height) == (160, 120):
            assert paths == ["tiles"] * 4                       # (~500 voxels per 4096 points: the tile path accepts every frame)
        for i in range(4):
            assert a[i].stage0_path() == paths[i], i
            assert a[i].launch_shape() == b[i].launch_shape() and a[i].launch_shape()[2] == 4
            assert_records(a[i].points(), frs[i]["records"], i)
            ref = dict(result=b[i].result, labels=want[i], debug={w: b[i].debug(w) for w in ALL_DEBUG})
            assert_same_frame(a[i], got[i], ref, (width, height, i))
        rc, olab, ores, oh = oracle.segment(frs[1]["records"], prm)
        assert rc == 0 and np.array_equal(got[1], olab)
        assert first_mismatch("MERGES", oh.get("MERGES"), a[1].debug("MERGES")) is None
        oh.close()
    finally:
        for c in a + b:
            c.close()


# ---- 3. narrow launches ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("width,height", [(67, 45), WIDE, (160, 120)])
def test_narrow_launches(P, gpu_ctx, point_runs, frames, monkeypatch, width, height, cap):
    """At one workgroup per frame d_deproject's loop goes round 75 times on 160 x 120 pixels and ends on a full trip; 67 x 45 and 4099 x 3 end on ragged ones."""
    fr = frames[(width, height, 7)]
    prm = params_for(P, width, height)
    ref = point_runs.get(fr["records"], prm)                    # (at the default width)
    assert ref["rc"] == 0
    monkeypatch.setenv("F3DS_GRID_CAP", str(cap))
    labels = gpu_ctx.segment_rgbd(fr["depth"], fr["color"], fr["fmt"], prm)
    assert gpu_ctx.launch_shape() == (cap, cap, 1)
    assert_records(gpu_ctx.points(), fr["records"], (width, height, cap))
    assert np.array_equal(labels, ref["labels"]) and not same_results(gpu_ctx.result, ref["result"])


# ---- 4. the context afterwards --------------------------------------------------------------------------------------------------------------------

def test_later_calls_answer_as_after_segment(P, gpu_ctx, ref_ctx, frames):
    fr = frames[(160, 120, 7)]
    prm = params_for(P, 160, 120)
    la = gpu_ctx.segment_rgbd(fr["depth"], fr["color"], fr["fmt"], prm)
    lb = ref_ctx.segment(fr["records"], prm)
    assert np.array_equal(la, lb)
    truth = synthetic_truth(fr["records"])                      # one label per pixel
    thr = np.array([0.2, 0.05, 0.12, 0.0], np.float32)
    (sa, na), (sb, nb) = gpu_ctx.evaluate_levels(truth, thr), ref_ctx.evaluate_levels(truth, thr)
    assert [s.as_dict() for s in sa] == [s.as_dict() for s in sb] and np.array_equal(na, nb)
    (va, ra), (vb, rb) = gpu_ctx.labels_at_thresholds(thr), ref_ctx.labels_at_thresholds(thr)
    assert np.array_equal(va, vb) and np.array_equal(ra, rb)
    assert gpu_ctx.evaluate(truth).as_dict() == ref_ctx.evaluate(truth).as_dict()
    prm2 = prm.copy(); prm2.threshold = 0.12; prm2.color_metric = P.RGB_EUCL
    assert np.array_equal(gpu_ctx.recluster(prm2), ref_ctx.recluster(prm2))
    assert not same_results(gpu_ctx.result, ref_ctx.result)
    ga, gb = gpu_ctx.regions(), ref_ctx.regions()
    assert sorted(ga) == sorted(gb) and len(ga["label"]) == gpu_ctx.result.n_regions
    for k in ga:
        assert same_bits(ga[k], gb[k]), k
    assert_records(gpu_ctx.points(), fr["records"], "after the later calls")


def test_point_and_rgbd_calls_alternate_on_one_context(P, point_runs, frames):
    big, small = frames[(160, 120, 8)], frames[(67, 45, 9)]
    prm = params_for(P, 67, 45)
    want_big, want_small = point_runs.get(big["records"], prm), point_runs.get(small["records"], prm)
    ctx = P.Context(0)
    try:
        assert np.array_equal(ctx.segment_rgbd(big["depth"], big["color"], big["fmt"], prm), want_big["labels"])
        assert np.array_equal(ctx.segment(small["records"], prm), want_small["labels"]) and not same_results(ctx.result, want_small["result"])
        assert_records(ctx.points(), small["records"], "host points are the context's too")
        assert np.array_equal(ctx.segment_rgbd(small["depth"], small["color"], small["fmt"], prm), want_small["labels"])
        assert np.array_equal(ctx.segment(big["records"], prm), want_big["labels"])
        assert np.array_equal(ctx.segment_rgbd(big["depth"], big["color"], big["fmt"], prm), want_big["labels"]) and not same_results(ctx.result, want_big["result"])
        assert_records(ctx.points(), big["records"], "rgbd after points")
    finally:
        ctx.close()


def test_get_points_refuses_what_the_context_does_not_own(P, frames):
    fr = frames[(67, 45, 7)]
    prm = params_for(P, 67, 45)
    ctx = P.Context(0)
    try:
        with pytest.raises(P.LogicError):
            ctx.points()                                        # nothing has run
        dev = to_device(fr["records"])
        ctx.segment(dev.data_ptr(), prm, n=len(fr["records"]), on_device=True)
        n = ctypes.c_size_t(12345)
        assert ctx.lib.f3ds_get_points(ctx.handle, None, 0, 0, ctypes.byref(n)) == P.ERR_LOGIC      # the caller's device buffer
        ctx.segment_rgbd(fr["depth"], fr["color"], fr["fmt"], prm)
        assert ctx.lib.f3ds_get_points(ctx.handle, None, 0, 0, ctypes.byref(n)) == 0 and n.value == 67 * 45
        out = np.zeros((67 * 45, 4), np.float32)
        assert ctx.lib.f3ds_get_points(ctx.handle, out.ctypes.data, 67 * 45 - 1, 0, ctypes.byref(n)) == P.ERR_CAPACITY
        dst = to_device(np.zeros((67 * 45, 4), np.float32))
        assert ctx.lib.f3ds_get_points(ctx.handle, ctypes.c_void_p(dst.data_ptr()), 67 * 45, 1, None) == 0      # to a device buffer
        assert_records(dst.cpu().numpy(), fr["records"], "device destination")
    finally:
        ctx.close()


# ---- 5. frames without a valid pixel ---------------------------------------------------------------------------------------------------------------

def test_all_invalid_frame(P, gpu_ctx, point_runs, frames):
    fr = frames[(67, 45, 7)]
    prm = params_for(P, 67, 45)
    nothing = np.zeros_like(fr["depth"])
    labels = gpu_ctx.segment_rgbd(nothing, fr["color"], fr["fmt"], prm)      # F3DS_OK (no exception)
    assert len(labels) == 67 * 45 and (labels == P.NO_LABEL).all()
    assert (gpu_ctx.result.n_points, gpu_ctx.result.n_finite, gpu_ctx.result.n_voxels, gpu_ctx.result.n_regions) == (67 * 45, 0, 0, 0)
    pts = gpu_ctx.points()
    assert np.isnan(pts[:, :3]).all() and np.array_equal(pts[:, 3].view(np.uint32), fr["records"][:, 3].view(np.uint32))
    frs = [frames[(67, 45, s)] for s in (7, 8, 9, 10)]
    depths = [f["depth"] for f in frs]; depths[2] = nothing
    ctxs = [P.Context(0) for _ in range(4)]
    try:
        got = P.segment_rgbd_batch(ctxs, depths, [f["color"] for f in frs], frs[0]["fmt"], prm)
        assert (got[2] == P.NO_LABEL).all() and ctxs[2].result.n_regions == 0 and ctxs[2].result.n_points == 67 * 45
        for i in (0, 1, 3):
            ref = point_runs.get(frs[i]["records"], prm)
            assert np.array_equal(got[i], ref["labels"]) and not same_results(ctxs[i].result, ref["result"]), i
    finally:
        for c in ctxs:
            c.close()


# ---- 6. the frame pipeline -------------------------------------------------------------------------------------------------------------------------

def test_stream_mixes_point_and_rgbd_frames(P, point_runs, frames):
    prm = params_for(P, 67, 45)
    order = [(160, 120, 7), (67, 45, 7), (67, 45, 8), (160, 120, 8), (160, 120, 9), (67, 45, 9)]      # submit, submit_rgbd, submit, ... of two sizes
    want = [point_runs.get(frames[k]["records"], prm) for k in order]
    got = []
    with P.FrameStream(0, depth=3) as fs:
        for i, k in enumerate(order):
            fr = frames[k]
            send = (lambda: fs.submit(fr["records"], prm, 100 + i)) if i % 2 == 0 else (lambda: fs.submit_rgbd(fr["depth"], fr["color"], fr["fmt"], prm, 100 + i))
            while not send():
                got.append(fs.next())                           # the pipeline is full: take the oldest frame (blocks until it is done)
        while fs.pending():
            got.append(fs.next())
        assert fs.next() is None
    assert [g[0] for g in got] == [100 + i for i in range(6)]  # in submission order, with their tags
    for i, (tag, labels, res) in enumerate(got):
        assert np.array_equal(labels, want[i]["labels"]), i
        assert not same_results(res, want[i]["result"]), i
