"""The 4x4x4 block arithmetic of the neighbour search (csrc/f3ds_numerics.h: n_block_key, n_block_cell, n_block_ordinal) without a GPU: the g++ build of the header
(tests/blockprobe/) runs the search the way the device does -- one (base ordinal, occupancy mask) per block, ordinal = base + popcount -- and a plain dictionary of the
keys is the reference.  Both leaf orders, depth 3, 10 and 12 (the deepest grid the block table serves)."""
import ctypes
import os

import numpy as np
import pytest

from block_table_common import brute_neighbors, in_leaf_order, morton
from conftest import ROOT, _make

VP = ctypes.c_void_p
DEPTHS = (3, 10, 12)


@pytest.fixture(scope="session")
def probe():
    _make("tests/blockprobe")          # (a no-op when the library is newer than its sources)
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "blockprobe", "libf3ds_blockprobe.so"))
    lib.bp_key.restype = ctypes.c_uint32; lib.bp_cell.restype = ctypes.c_uint
    lib.bp_ordinal.restype = ctypes.c_int; lib.bp_ordinal.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint, ctypes.c_int]
    lib.bp_neighbors.restype = ctypes.c_int
    return lib


def run(probe, keys, depth, leaf_order):
    """keys (any order, duplicates allowed) -> (keys in leaf order, the probe's V x 27 table)"""
    k = in_leaf_order(keys, depth, leaf_order)
    out = np.zeros((len(k), 27), np.int32)
    rc = probe.bp_neighbors(VP(k.ctypes.data), ctypes.c_uint32(len(k)), ctypes.c_int(depth), ctypes.c_int(leaf_order), VP(out.ctypes.data))
    assert rc == 0, rc
    return k, out


def check(probe, keys, depth, leaf_order):
    k, got = run(probe, keys, depth, leaf_order)
    want = brute_neighbors(k, (1 << depth) - 1)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "depth %d order %d: %d slots differ, first: voxel %s slot %d: %d vs %d" % (
        depth, leaf_order, len(bad), k[bad[0][0]].tolist(), bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])
    assert (got[:, 13] == np.arange(len(k))).all()          # slot 13 is the voxel itself
    return k, got


def cube(lo, hi):
    r = np.arange(lo, hi)
    return np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)


def test_cell_index_is_the_low_six_bits_of_the_leaf_sort(probe):
    """n_block_cell == Morton code & 63, n_block_key == the three keys >> 2 at ten bits each: cells of one block are then consecutive in either leaf order."""
    rng = np.random.default_rng(1)
    for depth in DEPTHS:
        k = rng.integers(0, 1 << depth, (500, 3)).astype(np.uint32)
        k[:8] = [(0, 0, 0), ((1 << depth) - 1,) * 3, (3, 3, 3), (4, 4, 4), (3, 4, 3), (0, 0, 1), (0, 1, 0), (1, 0, 0)]
        code = morton(k, depth)
        for (x, y, z), c in zip(k.tolist(), code.tolist()):
            assert probe.bp_cell(x, y, z) == c & 63
            assert probe.bp_key(x, y, z) == ((x >> 2) << 20) | ((y >> 2) << 10) | (z >> 2)
    assert [probe.bp_cell(*p) for p in ((0, 0, 1), (0, 1, 0), (1, 0, 0), (3, 3, 3))] == [1, 2, 4, 63]


def test_ordinal_at_the_ends_of_the_mask(probe):
    """cell 0 and cell 63, full and single-bit masks, both orders: no shift by 64, an empty cell answers -1"""
    full = (1 << 64) - 1
    for cell in range(64):
        assert probe.bp_ordinal(100, full, cell, 0) == 100 + cell
        assert probe.bp_ordinal(100, full, cell, 1) == 100 + 63 - cell
        assert probe.bp_ordinal(7, 1 << cell, cell, 0) == 7 and probe.bp_ordinal(7, 1 << cell, cell, 1) == 7
        assert probe.bp_ordinal(7, full ^ (1 << cell), cell, 0) == -1 and probe.bp_ordinal(7, full ^ (1 << cell), cell, 1) == -1
    assert probe.bp_ordinal(0, 0, 0, 0) == -1 and probe.bp_ordinal(0, 0, 63, 1) == -1
    assert probe.bp_ordinal(0xFFFFFF00, (1 << 63) | 1, 63, 0) == 0xFFFFFF00 - (1 << 32) + 1          # (the ordinal is the 32-bit sum)
    rng = np.random.default_rng(2)
    for _ in range(2000):
        mask = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)); cell = int(rng.integers(0, 64)); base = int(rng.integers(0, 1 << 30))
        below = bin(mask & ((1 << cell) - 1)).count("1"); above = bin(mask >> (cell + 1)).count("1")
        present = (mask >> cell) & 1
        assert probe.bp_ordinal(base, mask, cell, 0) == (base + below if present else -1)
        assert probe.bp_ordinal(base, mask, cell, 1) == (base + above if present else -1)


@pytest.mark.parametrize("leaf_order", [0, 1])
@pytest.mark.parametrize("depth", DEPTHS)
def test_neighbours_equal_a_dictionary_lookup(probe, depth, leaf_order):
    mk = (1 << depth) - 1
    top = mk - 3                                   # first key of the last block on an axis
    # a full block (cell 63, popcounts of an all-ones mask), alone and with all its 26 neighbour blocks full too
    k, got = check(probe, cube(4, 8) if depth > 2 else cube(0, 4), depth, leaf_order)
    assert len(k) == 64 and sorted(got[:, 13].tolist()) == list(range(64))
    if depth > 3:
        k, got = check(probe, cube(0, 12), depth, leaf_order)
        inner = ((k >= 4) & (k < 8)).all(1)
        assert (got[inner] >= 0).all()
    check(probe, cube(top, mk + 1), depth, leaf_order)          # the full block at the grid's upper corner
    # a single voxel: in the middle, at key 0, at max_key
    for p in ((5, 6, 3), (0, 0, 0), (mk, mk, mk), (0, mk, 3), (mk, 0, 4)):
        k, got = check(probe, [p], depth, leaf_order)
        assert (got[0] == np.where(np.arange(27) == 13, 0, -1)).all()
    # both sides of every block border: keys 3 | 4 on each axis and diagonally, alone and in pairs
    border = cube(3, 5)
    check(probe, border, depth, leaf_order)
    for i in range(len(border)):
        for j in range(i + 1, len(border)):
            k, got = check(probe, border[[i, j]], depth, leaf_order)
            assert (got >= 0).sum() == 4          # each sees itself and the other
    check(probe, np.concatenate([cube(2, 6), cube(3, 5) + [0, 0, 1]]), depth, leaf_order)
    # key 0 and max_key: out-of-grid neighbours are -1 even where wrapping the key around would find a voxel
    faces = np.concatenate([cube(0, 2), cube(mk - 1, mk + 1), [(0, mk, 0), (mk, 0, mk), (0, 0, mk), (mk, mk, 0)]])
    k, got = check(probe, faces, depth, leaf_order)
    zero = int(np.nonzero((k == 0).all(1))[0][0]); last = int(np.nonzero((k == mk).all(1))[0][0])
    assert (got[zero, [0, 1, 3, 4, 9, 10, 12]] == -1).all() and (got[last, [26, 25, 23, 22, 17, 16, 14]] == -1).all()
    # random sparse sets: scattered over the grid, and dense inside a few blocks
    rng = np.random.default_rng(100 * depth + leaf_order)
    for it in range(300):
        n = int(rng.integers(1, 200))
        if it % 3 == 0:
            keys = rng.integers(0, mk + 1, (n, 3))
        elif it % 3 == 1:
            keys = np.clip(rng.integers(0, mk + 1, 3) + rng.integers(-6, 7, (n, 3)), 0, mk)
        else:
            keys = np.concatenate([rng.integers(0, min(mk + 1, 9), (n, 3)), np.clip(mk - rng.integers(0, 9, (n, 3)), 0, mk)])
        check(probe, keys, depth, leaf_order)


def test_probe_refuses_what_the_table_does_not_serve(probe):
    k = np.array([[0, 0, 0], [8, 0, 0], [1, 0, 0]], np.uint32)          # the leaves of block 0 are not consecutive
    out = np.zeros((3, 27), np.int32)
    assert probe.bp_neighbors(VP(k.ctypes.data), ctypes.c_uint32(3), ctypes.c_int(10), ctypes.c_int(0), VP(out.ctypes.data)) == -2
    assert probe.bp_neighbors(VP(k.ctypes.data), ctypes.c_uint32(3), ctypes.c_int(13), ctypes.c_int(0), VP(out.ctypes.data)) == -1
