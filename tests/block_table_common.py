"""Shared by tests/test_block_table_cpu.py and tests/test_block_table_gpu.py: the neighbour search as a plain dictionary of voxel keys."""
import numpy as np

OFFSETS = np.array([(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)], np.int64)      # slot = (dx + 1) * 9 + (dy + 1) * 3 + dz + 1


def brute_neighbors(keys, max_key):
    """keys: V x 3 voxel keys, row v = leaf ordinal v.  Returns V x 27 int32: the ordinal of the leaf at key + offset, -1 where there is none or the cell lies outside [0, max_key]."""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    where = {tuple(k): v for v, k in enumerate(keys.tolist())}
    assert len(where) == len(keys), "a voxel key occurs twice"
    out = np.full((len(keys), 27), -1, np.int32)
    for s, d in enumerate(OFFSETS.tolist()):
        q = keys + np.array(d, np.int64)
        inside = ((q >= 0) & (q <= max_key)).all(1)
        out[:, s] = [where.get(tuple(k), -1) if ok else -1 for k, ok in zip(q.tolist(), inside.tolist())]
    return out


def morton(keys, depth):
    """Morton code of V x 3 keys: bit 3b + 2 of the code is bit b of x, 3b + 1 of y, 3b of z (the leaf sort's order)."""
    keys = np.asarray(keys, np.uint64).reshape(-1, 3)
    code = np.zeros(len(keys), np.uint64)
    for b in range(depth):
        for a in range(3):
            code |= ((keys[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - a)
    return code


def in_leaf_order(keys, depth, leaf_order):
    """The distinct keys in leaf order: ascending Morton code (leaf_order 0) or ascending complemented code, i.e. descending (1)."""
    keys = np.unique(np.asarray(keys, np.uint32).reshape(-1, 3), axis=0)
    o = np.argsort(morton(keys, depth), kind="stable")
    return np.ascontiguousarray(keys[o[::-1] if leaf_order == 1 else o])
