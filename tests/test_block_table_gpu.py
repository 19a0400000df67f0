"""The neighbour search of the device library against a plain dictionary of its own voxel keys (tests/block_table_common.py): VOXEL_NEIGHBORS must be, for every voxel
and each of the 27 offsets, the ordinal of the voxel at that key, -1 where there is none or the cell lies outside [0, max_key].  Grids of depth <= 12 go through the
4x4x4 block table (csrc/f3ds_kernels.inc, d_vox_table / bt_find), deeper ones through an entry per voxel; a lone frame takes stage 0's sort path (several workgroups
build the table), a batch of four the tile path (one workgroup per frame)."""
import numpy as np
import pytest

from block_table_common import brute_neighbors

pytestmark = pytest.mark.gpu
GRID = 32          # the hand-made cloud fills a grid of 32^3 cells (depth 5)


def cube(lo, hi):
    r = np.arange(lo, hi)
    return np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)


def handmade_voxels():
    rng = np.random.default_rng(41)
    parts = [cube(8, 12),                                                        # one block, full
             cube(2, 6),                                                         # both sides of the borders 3 | 4 on every axis, diagonals included
             np.array([(x, y, z) for x in (15, 16) for y in range(10, 21) for z in (12, 13)]),      # a sheet across 15 | 16, through several blocks
             cube(0, 2), np.array([(0, j, k) for j in range(0, 8) for k in range(0, 8)]),         # the grid's lower faces
             cube(GRID - 2, GRID), np.array([(GRID - 1, j, GRID - 1) for j in range(GRID - 8, GRID)]),      # and the upper ones
             rng.integers(0, GRID, (400, 3))]
    return np.unique(np.concatenate(parts), axis=0)


def handmade_cloud(res):
    """Three points in each voxel of handmade_voxels(), voxel after voxel; a point at the origin and the points inside cell 31 of every axis pin the grid: depth 5, keys == cell numbers."""
    vox = handmade_voxels()
    rng = np.random.default_rng(42)
    cells = np.repeat(vox, 3, axis=0).astype(np.float64) + 0.5 + rng.uniform(-0.2, 0.2, (3 * len(vox), 3))
    cells[0] = 0.0                                   # voxel (0, 0, 0) sorts first
    assert (vox[0] == 0).all() and (vox[-1] == GRID - 1).all()
    pts = np.zeros((len(cells), 4), np.float32)
    pts[:, :3] = (cells * res).astype(np.float32)
    pts[:, 3] = rng.integers(0, 2 ** 24, len(pts)).astype(np.uint32).view(np.float32)
    return pts, vox


def check(ctx, what):
    depth = int(ctx.result.octree_depth)
    keys = ctx.debug("VOXEL_KEYS").reshape(-1, 3)
    got = ctx.debug("VOXEL_NEIGHBORS").reshape(-1, 27)
    assert len(keys) == ctx.result.n_voxels and len(got) == len(keys) and len(keys) > 0, what
    want = brute_neighbors(keys, (1 << depth) - 1)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s (depth %d): %d of %d slots differ, first: voxel %d %s slot %d: %d vs %d" % (
        what, depth, len(bad), got.size, bad[0][0], keys[bad[0][0]].tolist(), bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])
    return keys, depth


@pytest.fixture(scope="module")
def organised(P):
    return [P.synth_frame(0, 7 + i, 160, 120, 30) for i in range(4)]


@pytest.mark.parametrize("leaf_order", [0, 1])
def test_organised_frame_alone(P, organised, leaf_order):
    ctx = P.Context(0)
    ctx.segment(organised[0], P.launch_params(voxel_res=0.02, seed_res=0.2, leaf_order=leaf_order))
    keys, depth = check(ctx, "lone frame")
    assert depth <= 12 and len(keys) > 64
    ctx.close()


@pytest.mark.parametrize("leaf_order", [0, 1])
def test_organised_frames_as_a_batch_of_four(P, organised, leaf_order):
    ctxs = [P.Context(0) for _ in organised]
    P.segment_batch(ctxs, organised, P.launch_params(voxel_res=0.02, seed_res=0.2, leaf_order=leaf_order))
    for i, c in enumerate(ctxs):
        check(c, "frame %d of the batch" % i)
        c.close()


@pytest.mark.parametrize("leaf_order", [0, 1])
def test_handmade_cloud(P, leaf_order):
    """a full block, voxels on both sides of block borders on all axes, voxels on the grid's lower and upper faces: alone and as a batch of four"""
    res = 0.01
    pts, vox = handmade_cloud(res)
    prm = P.launch_params(voxel_res=res, seed_res=4 * res, use_transform=0, leaf_order=leaf_order)
    ctxs = [P.Context(0) for _ in range(5)]
    ctxs[0].segment(pts, prm)
    P.segment_batch(ctxs[1:], [pts] * 4, prm)
    for i, c in enumerate(ctxs):
        keys, depth = check(c, "hand-made cloud, context %d" % i)
        assert depth == 5 and sorted(map(tuple, keys.tolist())) == sorted(map(tuple, vox.tolist()))      # the cloud is what it was made to be
        c.close()


@pytest.mark.parametrize("batch", [1, 4])
def test_deep_grid_takes_the_table_with_an_entry_per_voxel(P, batch):
    pts = P.synth_frame(0, 5, 120, 90, 20)
    prm = P.launch_params(voxel_res=0.00025, seed_res=0.0025)
    ctxs = [P.Context(0) for _ in range(batch)]
    if batch == 1:
        ctxs[0].segment(pts, prm)
    else:
        P.segment_batch(ctxs, [pts] * batch, prm)
    for c in ctxs[:2]:
        keys, depth = check(c, "deep grid")
        assert depth > 12
        c.close()
    for c in ctxs[2:]:
        c.close()
