"""The label tracker on the device (f3ds_tracker_update: d_track_keys, the stage-0 sort, the d_evl_* reduction, d_track_pack, d_track_apply in
csrc/f3ds_track.inc) against the numpy / Python reference of tests/track_common.py.  Every case compares the id image, Tracker.ids() and every field of
f3ds_track_result with the reference, exactly, after every frame.  Shapes: 97 x 61 u16 tight (5917 pixels: 23 full trips of a 256-lane workgroup and a ragged
one at F3DS_GRID_CAP=1), 67 x 45 f32 with padded rows, 3 x 2 and 1 x 1; the main cases run at the default launch width and at 1 and 3 workgroups."""
import ctypes

import numpy as np
import pytest

import track_common as T
from rgbd_common import DEPTH_PAD, frame_images, padded
from track_common import NO

pytestmark = pytest.mark.gpu
SHAPES = [(97, 61, "u16", "tight"), (67, 45, "f32", "padded"), (3, 2, "u16", "tight"), (1, 1, "f32", "tight")]
ONE = dict(min_votes=1, min_permille=300, depth_tol=0.05)


def to_device(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
    torch.cuda.synchronize()
    return t


def raw_update(P, trk, fmt, depth, labels, n_regions, pose, where="host", layout="tight"):
    """f3ds_tracker_update on raw buffers: (rc, ids image, result).  layout "padded": depth rows DEPTH_PAD bytes longer; where "device": every buffer on the GPU"""
    f = fmt.copy()
    depth = np.ascontiguousarray(depth)
    if layout == "padded":
        dbuf, f.depth_pitch = padded(depth, DEPTH_PAD["u16" if depth.dtype == np.uint16 else "f32"])
        dbuf = dbuf.reshape(-1)
    else:
        dbuf = depth.view(np.uint8).reshape(-1)
    lab = np.ascontiguousarray(labels, np.uint32).reshape(-1)
    n = int(fmt.width) * int(fmt.height)
    m = None if pose is None else np.ascontiguousarray(pose, np.float32)
    mp = None if m is None else m.ctypes.data
    res = P.TrackResult()
    if where == "device":
        import torch
        dd, dl, di = to_device(dbuf), to_device(lab.view(np.int32)), to_device(np.full(n, 0x5A5A5A5A, np.int32))
        rc = trk.lib.f3ds_tracker_update(trk.handle, ctypes.byref(f), ctypes.c_void_p(dd.data_ptr()), ctypes.c_void_p(dl.data_ptr()), n_regions, 1, mp,
                                         ctypes.c_void_p(di.data_ptr()), 1, ctypes.byref(res))
        torch.cuda.synchronize()
        ids = di.cpu().numpy().view(np.uint32)
    else:
        ids = np.full(n, 0x5A5A5A5A, np.uint32)
        rc = trk.lib.f3ds_tracker_update(trk.handle, ctypes.byref(f), dbuf.ctypes.data, lab.ctypes.data, n_regions, 0, mp, ids.ctypes.data, 0, ctypes.byref(res))
    return rc, ids, res


def step(P, trk, ref, fmt, fr, where="host", layout="tight"):
    """one frame through the tracker and the reference; everything compared; returns the reference's (rc, ids image, ids, result)"""
    before = None if trk_never_ran(trk) else trk.ids()
    rc, ids, res = raw_update(P, trk, fmt, fr["depth"], fr["labels"], fr["n_regions"], fr.get("pose"), where, layout)
    want = ref.update(fmt, fr["depth"], fr["labels"], fr["n_regions"], fr.get("pose"))
    assert rc == want[0], (rc, want[0])
    if rc == 0:
        assert np.array_equal(ids, want[1]), np.flatnonzero(ids != want[1])[:8]
        assert np.array_equal(trk.ids(), want[2])
        assert res.as_dict() == want[3], (res.as_dict(), want[3])
    elif before is not None:
        assert np.array_equal(trk.ids(), before)
    return want


def trk_never_ran(trk):
    n = ctypes.c_size_t()
    return trk.lib.f3ds_tracker_get_ids(trk.handle, None, 0, ctypes.byref(n)) == -5


def make(P, prm):
    return P.Tracker(0, P.TrackParams(prm["min_votes"], prm["min_permille"], prm["depth_tol"])), T.RefTracker(**prm)


def run(P, fmt, frames, prm=ONE, where="host", layout="tight"):
    trk, ref = make(P, prm)
    try:
        return [step(P, trk, ref, fmt, fr, where, layout) for fr in frames]
    finally:
        trk.close()


def scene(width, height, depth_kind, nx, ny, mm=None, seed=0):
    """blocks of nx * ny regions over planes 200 mm apart, 10 % holes, a few unlabelled pixels"""
    rng = np.random.default_rng(seed + width)
    lab = T.blocks(width, height, nx, ny)
    base = (1000.0 + 200.0 * lab) if mm is None else np.full((height, width), float(mm))
    base = np.where(rng.random((height, width)) < 0.10, 0.0, base)
    lab = np.where(rng.random((height, width)) < 0.05, np.uint32(NO), lab).astype(np.uint32)
    return dict(depth=T.to_depth(base, depth_kind), labels=lab, n_regions=nx * ny, pose=None)


def grid_of(width, height):
    return (max(1, min(4, width // 8)), max(1, min(3, height // 8)))


# ---- 1. the main cases, every shape, default and narrow launches ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [0, 1, 3])
@pytest.mark.parametrize("width,height,depth_kind,layout", SHAPES)
def test_first_same_permuted(P, monkeypatch, width, height, depth_kind, layout, cap):
    """a first frame gets fresh ids in region order; the same frame again keeps everything; renumbered labels give the same id image"""
    if cap:
        monkeypatch.setenv("F3DS_GRID_CAP", str(cap))
    fmt = T.track_format(P, width, height, depth_kind)
    nx, ny = grid_of(width, height)
    a = scene(width, height, depth_kind, nx, ny)
    K = a["n_regions"]
    perm = np.random.default_rng(5).permutation(K).astype(np.uint32)
    c = dict(a); c["labels"] = np.where(a["labels"] == NO, np.uint32(NO), perm[np.minimum(a["labels"], K - 1)]).astype(np.uint32)
    for where in ("host", "device"):
        r = run(P, fmt, [a, a, c], ONE, where, layout)
        first, again, renum = r
        present = np.unique(first[1][first[1] != NO])
        assert first[3]["first_frame"] == 1 and first[3]["n_votes"] == 0 and first[3]["n_matched"] == 0
        assert np.array_equal(present, np.arange(first[3]["n_new"]))                       # fresh ids, in region order
        assert np.array_equal(first[2][first[2] != NO], np.arange(first[3]["n_new"]))
        assert again[3]["first_frame"] == 0 and again[3]["n_new"] == 0 and again[3]["next_id"] == first[3]["next_id"] and again[3]["n_votes"] == again[3]["n_labelled"]
        assert np.array_equal(again[1], first[1]) and np.array_equal(renum[1], first[1]) and renum[3]["n_new"] == 0


@pytest.mark.parametrize("cap", [0, 1, 3])
def test_split_merge_and_the_permille_border(P, monkeypatch, cap):
    if cap:
        monkeypatch.setenv("F3DS_GRID_CAP", str(cap))
    w, h = 97, 61
    fmt = T.track_format(P, w, h)
    depth = np.full((h, w), 1500, np.uint16)
    two = np.zeros((h, w), np.uint32); two[:, 50:] = 1                       # region 0: 50 columns, region 1: 47
    split = two.copy(); split[:, 50:70] = 2; split[:, 70:] = 0              # the old region 1 in two parts: label 2 (20 columns) and label 0 (27), old region 0 now label 1
    split[:, :50] = 1
    merged = np.zeros((h, w), np.uint32)
    fr = lambda lab, K: dict(depth=depth, labels=lab, n_regions=K)
    r = run(P, fmt, [fr(two, 2), fr(split, 3), fr(merged, 1)], ONE)
    assert list(r[0][2]) == [0, 1]
    assert list(r[1][2]) == [1, 0, 2] and r[1][3]["n_new"] == 1 and r[1][3]["n_retired"] == 0      # the larger part (27 columns) keeps id 1
    assert list(r[2][2]) == [0] and r[2][3]["n_retired"] == 2 and r[2][3]["n_matched"] == 1        # id 0 had 50 columns of votes; ids 1 and 2 retire
    # a region fails min_permille by one vote: 1000 labelled pixels, 300 of them (at 300 permille: just enough) or 299 land on the old region
    for votes, keeps in ((300, True), (299, False)):
        prev = np.full((h, w), NO, np.uint32); prev.reshape(-1)[:votes] = 0
        cur = np.full((h, w), NO, np.uint32); cur.reshape(-1)[:1000] = 0
        r = run(P, fmt, [fr(prev, 1), fr(cur, 1)], ONE)
        assert r[1][3]["n_votes"] == votes and r[1][3]["n_labelled"] == 1000 and (r[1][3]["n_matched"] == 1) == keeps and list(r[1][2]) == [0 if keeps else 1]


@pytest.mark.parametrize("cap", [0, 1, 3])
def test_occlusion_holes_and_unlabelled_pixels(P, monkeypatch, cap):
    if cap:
        monkeypatch.setenv("F3DS_GRID_CAP", str(cap))
    w, h = 67, 45
    fmt = T.track_format(P, w, h, "f32")
    lab = np.zeros((h, w), np.uint32)
    far = dict(depth=T.to_depth(np.full((h, w), 2000.0), "f32"), labels=lab, n_regions=1)
    near = dict(depth=T.to_depth(np.full((h, w), 1500.0), "f32"), labels=lab, n_regions=1)
    r = run(P, fmt, [far, near], ONE, layout="padded")                       # a nearer plane in front: |1.5 - 2.0| > 0.05 * 1.5
    assert r[1][3]["n_votes"] == 0 and list(r[1][2]) == [1] and r[1][3]["n_retired"] == 1
    r = run(P, fmt, [far, near], dict(ONE, depth_tol=0.5), layout="padded")
    assert r[1][3]["n_votes"] == w * h and list(r[1][2]) == [0]
    # holes in either frame, unlabelled pixels with a depth, labelled pixels without one
    def holed(seed):
        g = np.random.default_rng(seed)
        d = np.where(g.random((h, w)) < 0.3, 0.0, 2000.0)
        l = np.where(g.random((h, w)) < 0.3, np.uint32(NO), T.blocks(w, h, 3, 2)).astype(np.uint32)
        return dict(depth=T.to_depth(d, "f32"), labels=l, n_regions=6)
    a, b = holed(1), holed(2)
    assert ((a["depth"] == 0) & (a["labels"] != NO)).any() and ((a["depth"] != 0) & (a["labels"] == NO)).any()
    r = run(P, fmt, [a, b, a], ONE, layout="padded")
    assert ((r[1][1] != NO) == (b["labels"].reshape(-1) != NO)).all()           # an id wherever there is a label, valid depth or not
    assert 0 < r[1][3]["n_votes"] < r[1][3]["n_labelled"] and r[1][3]["n_new"] == 0


def test_a_pose_that_shifts_the_plane_five_columns(P):
    w, h = 97, 61
    fmt = T.track_format(P, w, h)
    depth = np.full((h, w), 1500, np.uint16)
    prev = T.blocks(w, h, 4, 1)
    cur = np.roll(prev, -5, axis=1)                                             # what was at column u + 5 is now at column u ...
    pose = T.column_shift_pose(fmt, np.float32(1500) * np.float32(0.001), 5)    # ... and lands on column u + 5 of the previous frame
    r = run(P, fmt, [dict(depth=depth, labels=prev, n_regions=4), dict(depth=depth, labels=cur, n_regions=4, pose=pose)], ONE)
    assert r[1][3]["n_labelled"] == w * h and r[1][3]["n_votes"] == (w - 5) * h      # the five columns that leave the image count in size, not in the votes
    assert list(r[1][2]) == [0, 1, 2, 3]


def test_empty_frames_reset_and_errors_leave_the_state(P):
    w, h = 97, 61
    fmt = T.track_format(P, w, h)
    a = scene(w, h, "u16", 4, 3)
    nothing = dict(depth=np.zeros((h, w), np.uint16), labels=a["labels"], n_regions=12)
    no_regions = dict(depth=a["depth"], labels=np.full((h, w), NO, np.uint32), n_regions=0)
    trk, ref = make(P, ONE)
    try:
        with pytest.raises(P.LogicError):
            trk.ids()
        r0 = step(P, trk, ref, fmt, a)
        r1 = step(P, trk, ref, fmt, nothing)                                    # F3DS_OK, all ids F3DS_NO_LABEL wherever there is no label ...
        assert r1[0] == 0 and r1[3]["n_nonempty"] == 0 and r1[3]["n_retired"] == r0[3]["n_new"] and (r1[2] == NO).all()
        r2 = step(P, trk, ref, fmt, a)                                          # ... and the next frame matches nothing
        assert r2[3]["n_matched"] == 0 and r2[3]["first_frame"] == 0 and r2[2][r2[2] != NO].min() == r0[3]["next_id"]
        r3 = step(P, trk, ref, fmt, no_regions)
        assert r3[0] == 0 and len(r3[2]) == 0 and (r3[1] == NO).all()
        r4 = step(P, trk, ref, fmt, a)
        assert r4[3]["n_matched"] == 0
        # reset keeps next_id
        trk.reset(); ref.reset()
        r5 = step(P, trk, ref, fmt, a)
        assert r5[3]["first_frame"] == 1 and r5[2][r5[2] != NO].min() == r4[3]["next_id"]
        # another format: refused, the state intact
        other = T.track_format(P, w, h); other.fx = fmt.fx * 1.5
        assert step(P, trk, ref, other, a)[0] == P.ERR_ARG
        small = T.track_format(P, 67, 45)
        assert step(P, trk, ref, small, scene(67, 45, "u16", 2, 2))[0] == P.ERR_ARG
        # a label >= n_regions: found on the device, refused, the state intact -- the next update proves it
        bad = dict(a); bad["labels"] = a["labels"][::-1].copy(); bad["labels"][h - 1, w - 1] = 12
        bad["depth"] = np.where(a["depth"] > 0, a["depth"] + 1000, 0).astype(np.uint16)      # (a frame that would match nothing of `a` had it become the state)
        assert step(P, trk, ref, fmt, bad)[0] == P.ERR_ARG
        assert step(P, trk, ref, fmt, bad, where="device")[0] == P.ERR_ARG
        r6 = step(P, trk, ref, fmt, a)
        assert r6[3]["n_new"] == 0 and np.array_equal(r6[1], r5[1])
        # other argument errors
        lib, f = trk.lib, fmt
        d, l, o = a["depth"], a["labels"], np.zeros(w * h, np.uint32)
        good = [trk.handle, ctypes.byref(f), d.ctypes.data, l.ctypes.data, 12, 0, None, o.ctypes.data, 0, None]
        for k in (0, 1, 2, 3, 7):
            args = list(good); args[k] = None
            assert lib.f3ds_tracker_update(*args) == P.ERR_ARG, k
        pose = np.eye(3, 4, dtype=np.float32).reshape(12); pose[3] = np.inf
        args = list(good); args[6] = pose.ctypes.data
        assert lib.f3ds_tracker_update(*args) == P.ERR_ARG
        args = list(good); args[4] = 0x01000000
        assert lib.f3ds_tracker_update(*args) == P.ERR_UNSUPPORTED
        bad_fmt = fmt.copy(); bad_fmt.depth_scale = 0.0
        args = list(good); args[1] = ctypes.byref(bad_fmt)
        assert lib.f3ds_tracker_update(*args) == P.ERR_ARG
        n = ctypes.c_size_t()
        assert lib.f3ds_tracker_get_ids(trk.handle, o.ctypes.data, 11, ctypes.byref(n)) == P.ERR_CAPACITY and n.value == 12
        r7 = step(P, trk, ref, fmt, a)                                          # the tracker still works, and nothing above touched it
        assert r7[3]["n_new"] == 0 and np.array_equal(r7[1], r5[1])
    finally:
        trk.close()


def test_more_entries_than_the_first_download_holds(P):
    """every pixel its own region: 5917 (region, slot) pairs, more than the update's first download has room for"""
    w, h = 97, 61
    fmt = T.track_format(P, w, h)
    lab = np.arange(w * h, dtype=np.uint32).reshape(h, w)
    fr = dict(depth=np.full((h, w), 1200, np.uint16), labels=lab, n_regions=w * h)
    back = dict(fr); back["labels"] = lab[::-1, ::-1].copy()
    r = run(P, fmt, [fr, fr, back, fr], ONE)
    assert r[1][3]["n_entries"] == w * h and r[1][3]["n_matched"] == w * h and np.array_equal(r[2][1], r[0][1]) and r[3][3]["n_new"] == 0


def test_three_trackers_interleaved(P):
    w, h = 67, 45
    fmt = T.track_format(P, w, h)
    seqs = [[scene(w, h, "u16", 3, 2, seed=s), scene(w, h, "u16", 2, 3, seed=s + 10), scene(w, h, "u16", 3, 2, seed=s)] for s in (1, 2, 3)]
    pairs = [make(P, ONE) for _ in seqs]
    try:
        for k in range(3):
            for (trk, ref), frames in zip(pairs, seqs):
                step(P, trk, ref, fmt, frames[k], where="device" if k == 1 else "host")
    finally:
        for trk, _ in pairs:
            trk.close()


# ---- 2. seeded random sequences ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def random_runs(P):
    return {seed: (T.random_sequence(P, seed),) + T.run_reference(T.random_sequence(P, seed)) for seed in T.RANDOM_SEEDS}


def test_the_random_sequences_reach_every_branch(random_runs):
    reached = {k: sum(1 for _, _, c in random_runs.values() if c.get(k)) for k in T.BRANCHES}
    assert all(v >= 1 for v in reached.values()), reached


@pytest.mark.parametrize("seed", T.RANDOM_SEEDS)
def test_random_sequence(P, monkeypatch, random_runs, seed):
    seq, want, _ = random_runs[seed]
    if seed % 4 == 3:
        monkeypatch.setenv("F3DS_GRID_CAP", "1" if seed % 8 == 3 else "3")
    got = run(P, seq["fmt"], seq["frames"], seq["params"], "device" if seed % 3 == 1 else "host", "padded" if seed % 2 else "tight")
    for g, w in zip(got, want):                                                 # (run() compared the device with a fresh reference; this ties it to the shared one)
        assert g[0] == w[0] == 0 and np.array_equal(g[1], w[1]) and g[3] == w[3]


# ---- 3. end to end: segment_rgbd into a tracker -------------------------------------------------------------------------------------------------------------

def test_segmented_frames_keep_their_ids(P, gpu_ctx):
    fmt, depth, color = frame_images(P, 7, 160, 120)
    prm = P.launch_params(voxel_res=0.02, seed_res=0.2)
    n = 160 * 120
    one = P.default_track_params(min_votes=1)                                  # (a segmenter's smallest regions are a few pixels)
    with P.Tracker(0, one) as trk:
        ref = T.RefTracker(min_votes=1)
        lab1 = gpu_ctx.segment_rgbd(depth, color, fmt, prm); K1 = gpu_ctx.result.n_regions
        ids1 = trk.update(depth, lab1, K1, fmt)
        lab2 = gpu_ctx.segment_rgbd(depth, color, fmt, prm); K2 = gpu_ctx.result.n_regions
        ids2 = trk.update(depth, lab2, K2, fmt)
        assert K1 > 10 and np.array_equal(ids2, ids1) and trk.result.n_new == 0 and trk.result.n_matched == trk.result.n_nonempty
        w1 = ref.update(fmt, depth, lab1, K1); w2 = ref.update(fmt, depth, lab2, K2)
        assert np.array_equal(ids1, w1[1]) and np.array_equal(ids2, w2[1]) and trk.result.as_dict() == w2[3]
    # the same with every buffer on the device: the images, the labels segment_rgbd writes, the ids
    import torch
    dd, dc = to_device(depth.view(np.uint8)), to_device(color)
    dl, di = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    with P.Tracker(0, one) as trk:
        for want in (ids1, ids2):
            gpu_ctx.segment_rgbd(dd.data_ptr(), dc.data_ptr(), fmt, prm, labels_out=dl.data_ptr(), on_device=True)
            trk.update(dd.data_ptr(), dl.data_ptr(), gpu_ctx.result.n_regions, fmt, ids_out=di.data_ptr(), on_device=True)
            torch.cuda.synchronize()
            assert np.array_equal(di.cpu().numpy().view(np.uint32), want)
