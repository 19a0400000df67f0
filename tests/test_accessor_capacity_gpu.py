"""The capacity protocol of the accessors, through the raw C entry points: every f3ds_get_* reports its count with all outputs null, fills exactly what the
Python getter returns at cap = n, and at cap = n - 1 returns F3DS_ERR_CAPACITY with the count still reported.  A streaming accessor (its count comes out
of the walk) has then filled the first n - 1 entries; an all-or-nothing accessor (its count is known up front) has written nothing.  One frame, the one of
smoke(): synth_frame(0, 7, 160, 120, 30) at voxel_res 0.02, seed_res 0.2."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
U, F, F3, U2 = (np.uint32, ()), (np.float32, ()), (np.float32, (3,)), (np.uint32, (2,))
SENTINEL = 0xA5
# name -> (outputs in the C signature's order, streaming?, the Python getter's arrays in that order)
ACCESSORS = {
    "regions": ([U, U, F3, F3, F3], True, lambda c, r: [c.regions()[k] for k in ("label", "n_voxels", "xyz", "normal", "rgb")]),
    "region_voxels": ([F3, U, U], True, lambda c, r: list(c.region_voxels())),
    "voxel_cloud": ([F3, U, U], True, lambda c, r: list(c.voxel_cloud())),
    "voxel_centroid_cloud": ([F3, U, U], False, lambda c, r: list(c.voxel_centroid_cloud())),
    "supervoxels": ([U, F3, F3, F3, U], True, lambda c, r: [c.supervoxels()[k] for k in ("label", "xyz", "rgb", "normal", "n_voxels")]),
    "refined_voxels": ([U, F3], False, lambda c, r: [r["voxel_label"], r["voxel_normal"]]),
    "refined_supervoxels": ([U, F3, F3, F3, U], True, lambda c, r: [r[k] for k in ("label", "xyz", "rgb", "normal", "n_voxels")]),
    "supervoxel_adjacency": ([U2], False, lambda c, r: [c.supervoxel_adjacency()]),
    "region_adjacency": ([U2], False, lambda c, r: [c.region_adjacency()]),
    "merge_tree": ([U, U, F], False, lambda c, r: list(c.merge_tree())),
}


def c_entry(ctx, name):
    return getattr(ctx.lib, "f3ds_get_" + name)


def raw(ctx, name, bufs, cap):
    """(rc, n_out) of one call of the C accessor; bufs: an array or None per output"""
    n = ctypes.c_size_t(0xDEAD)
    rc = c_entry(ctx, name)(ctx.handle, *[None if b is None else b.ctypes.data for b in bufs], cap, ctypes.byref(n))
    return rc, n.value


def sentinel_buffers(outs, n):
    bufs = [np.empty((n,) + shape, dt) for dt, shape in outs]
    for b in bufs:
        b.view(np.uint8)[...] = SENTINEL
    return bufs


@pytest.fixture(scope="module")
def state(P):
    """the segmented and once-refined frame, and what every Python getter returns for it"""
    ctx = P.Context(0)
    ctx.segment(P.synth_frame(0, 7, 160, 120, 30), P.launch_params(voxel_res=0.02, seed_res=0.2))
    refined = ctx.refine_supervoxels(1)
    want = {name: spec[2](ctx, refined) for name, spec in ACCESSORS.items()}
    yield ctx, want
    ctx.close()


@pytest.mark.parametrize("name", sorted(ACCESSORS))
def test_count_fill_and_capacity(P, state, name):
    ctx, want = state
    outs, streaming, _ = ACCESSORS[name]
    want = want[name]
    n = len(want[0])
    assert n >= 2 and all(len(w) == n for w in want)
    # all outputs null: the count alone
    assert raw(ctx, name, [None] * len(outs), 0) == (P.OK, n)
    # cap = n, every output: the getter's arrays
    full = sentinel_buffers(outs, n)
    assert raw(ctx, name, full, n) == (P.OK, n)
    for k, (g, w) in enumerate(zip(full, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (name, k)
    # cap = n - 1, one output at a time: CAPACITY, the count still reported
    for k in range(len(outs)):
        bufs = sentinel_buffers(outs, n)
        rc, got_n = raw(ctx, name, [b if j == k else None for j, b in enumerate(bufs)], n - 1)
        assert (rc, got_n) == (P.ERR_CAPACITY, n), (name, k)
        b = bufs[k]
        if streaming:      # the first n - 1 entries are there, the last one was never touched
            assert b[:n - 1].tobytes() == full[k][:n - 1].tobytes(), (name, k)
            assert (b[n - 1:].view(np.uint8) == SENTINEL).all(), (name, k)
        else:
            assert (b.view(np.uint8) == SENTINEL).all(), (name, k)
        for j, o in enumerate(bufs):      # (and no output that was not asked for)
            assert j == k or (o.view(np.uint8) == SENTINEL).all()


def test_logic_errors_of_the_prologue(P):
    """The refined state does not exist before a refinement; caller-supplied supervoxels have no voxel grid."""
    prm = P.launch_params(voxel_res=0.02, seed_res=0.2)
    ctx = P.Context(0)
    try:
        ctx.segment(P.synth_frame(0, 7, 160, 120, 30), prm)
        for name in ("refined_voxels", "refined_supervoxels"):
            assert raw(ctx, name, [None] * len(ACCESSORS[name][0]), 0)[0] == P.ERR_LOGIC
        assert raw(ctx, "voxel_centroid_cloud", [None] * 3, 0)[0] == P.OK
        segm = {7: dict(voxels_xyz=[[0, 0, 1]], voxels_rgba=[0x00FF0000], centroid=[0, 0, 1], normal=[0, 0, 1]),
                9: dict(voxels_xyz=[[0.02, 0, 1]], voxels_rgba=[0x0000FF00], centroid=[0.02, 0, 1], normal=[0, 0, 1])}
        ctx.cluster_supervoxels(P.pack_supervoxels(segm), [(7, 9)], prm)
        assert raw(ctx, "voxel_centroid_cloud", [None] * 3, 0)[0] == P.ERR_LOGIC
        assert raw(ctx, "supervoxels", [None] * 5, 0) == (P.OK, 2)
    finally:
        ctx.close()
