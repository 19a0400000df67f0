"""Shared by tests/test_eval_levels_api_cpu.py and tests/test_eval_levels_gpu.py: the g++ harness of csrc/f3ds_eval_levels.h, the dense
contingency table of a segmentation built from public outputs only (the construction of test_evaluation.py::
test_oracle_evaluate_against_numpy, vectorised), and a numpy restatement of the rule that turns a frame's base table into level tables."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT

HARNESS_SRC = os.path.join(ROOT, "tests", "eval_levels_harness", "eval_levels_harness.cpp")
FIELDS = ("voi", "precision", "recall", "fscore", "wov", "fpr", "fnr")
NO_LABEL = 0xFFFFFFFF


def build_harness(directory):
    out = os.path.join(str(directory), "libeval_levels_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, HARNESS_SRC], check=True)
    lib = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    lib.evl_check.argtypes = [ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint32, vp]
    lib.evl_check.restype = None
    return lib


def harness_scores(lib, table, ssize, tsize, N):
    """(dense routine, sparse routine with std::log, sparse routine with m_logf): three float32[7] in FIELDS order."""
    table = np.ascontiguousarray(table, np.uint32)
    K, M = table.shape
    ssize = np.ascontiguousarray(ssize, np.uint32)
    tsize = np.ascontiguousarray(tsize, np.uint32)
    out = np.zeros(21, np.float32)
    lib.evl_check(K, M, table.ctypes.data, ssize.ctypes.data, tsize.ctypes.data, int(N), out.ctypes.data)
    return out[:7], out[7:14], out[14:]


def bits(perf):
    """the seven scores of a Performance record as uint32 bit patterns"""
    return np.array([getattr(perf, f) for f in FIELDS], np.float32).view(np.uint32).tolist()


def voxel_truth_labels(point_voxel, voxel_count, truth, P):
    """Truth label of every voxel as main() builds it: mean label colour per voxel, numbered by first appearance."""
    pv = np.asarray(point_voxel)
    V = len(voxel_count)
    lut = np.array([P.label_color(i) for i in range(256)], np.uint32)[np.asarray(truth) % 256]
    sums = np.zeros((V, 3), np.float64)
    ok = pv >= 0
    for k, sh in enumerate((16, 8, 0)):
        np.add.at(sums[:, k], pv[ok], ((lut[ok] >> sh) & 255).astype(np.float64))
    cnt = np.asarray(voxel_count).astype(np.float32)
    mean = (sums.astype(np.float32) / cnt[:, None]).astype(np.uint32)
    col = (mean[:, 0] << 16) | (mean[:, 1] << 8) | mean[:, 2]
    _, first, inv = np.unique(col, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.uint32)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first), dtype=np.uint32)
    return rank[inv].astype(np.uint32)


def cloud_voxels(cloud_xyz, voxel_xyz):
    """index into voxel_xyz of every row of cloud_xyz (voxel centroids are distinct points)"""
    key = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1, 3).view(np.dtype((np.void, 12))).ravel()
    vk, ck = key(voxel_xyz), key(cloud_xyz)
    order = np.argsort(vk, kind="stable")
    svk = vk[order]
    assert len(np.unique(svk)) == len(svk)
    pos = np.searchsorted(svk, ck)
    assert np.all(svk[np.clip(pos, 0, len(svk) - 1)] == ck)
    return order[pos]


def dense_table(cloud_xyz, cloud_seg, voxel_xyz, tl):
    """(table K x M, ssize, tsize, repeats): the contingency table of a labelled voxel cloud against per-voxel truth labels; a point that a ghost
    leaf repeats inside one segment counts once in the table and every time in ssize.  repeats = the number of such repeated points."""
    seg = np.asarray(cloud_seg, np.int64)
    v = cloud_voxels(cloud_xyz, voxel_xyz)
    K, M = int(seg.max()) + 1, int(tl.max()) + 1
    V = len(voxel_xyz)
    pairs = np.unique(seg * V + v)
    table = np.zeros((K, M), np.uint32)
    np.add.at(table, (pairs // V, tl[pairs % V]), 1)
    return table, np.bincount(seg, minlength=K).astype(np.uint32), np.bincount(tl, minlength=M).astype(np.uint32), len(seg) - len(pairs)


def level_table_numpy(base, tab_l, ghosts, owner, tl, K, M):
    """The level-table rule of csrc/f3ds_eval_levels.inc (d_evl_level_keys) restated: base = rows (supervoxel h, truth label j, count) of the
    frame's base table, tab_l[h] = the region of supervoxel h at this level, ghosts = rows (supervoxel h, voxel v) of the live ghost leaves,
    owner[v] = the supervoxel that owns voxel v (0: none), tl[v] = the truth label of voxel v.  Returns (table K x M, ssize)."""
    table = np.zeros((K, M), np.uint32)
    ssize = np.zeros(K, np.uint32)
    for h, j, c in base:
        table[tab_l[h], j] += c
        ssize[tab_l[h]] += c
    for h, v in ghosts:
        i = tab_l[h]
        ssize[i] += 1                                                       # a ghost leaf always adds to its segment's size ...
        seen = owner[v] != 0 and tab_l[owner[v]] == i                       # ... and to the intersection unless the voxel is in the segment already:
        seen = seen or any(g < h and gv == v and tab_l[g] == i for g, gv in ghosts)      # through its owner, or through an earlier ghost leaf
        if not seen:
            table[i, tl[v]] += 1
    return table, ssize


def best_level_rule(thresholds, fscores):
    """Clustering::best_thresh (src/clustering.cpp:759-774) over a std::map<float, performanceSet>: ascending thresholds, the first inserted of
    equal keys, the first strictly greater F-score starting from 0.  Returns the index into the given lists, or -1."""
    first = {}
    for l, t in enumerate(thresholds):
        first.setdefault(float(np.float32(t)), l)
    best, bf = -1, np.float32(0)
    for t in sorted(first):
        l = first[t]
        if np.float32(fscores[l]) > bf:
            best, bf = l, np.float32(fscores[l])
    return best


SEEN_SEEDS = (1777, 1928, 2274)


def seen_cloud(P, seed):
    """(points, params, truth): a small seeded cloud whose run to threshold 1 ends with a ghost leaf inside the segment that already holds its
    voxel (voxel_cloud() repeats a point inside one segment): the "seen" branch of the ghost rule.  Found by a search over seeds 0 .. 2499 of
    this generator with the oracle (463 runs ended with live ghost leaves, three with a repeat: SEEN_SEEDS)."""
    rng = np.random.default_rng(seed)
    kind = int(rng.integers(0, 5))
    n = int(rng.choice([50, 400, 3000]))
    s = float(rng.choice([0.1, 1.0]))
    xyz = rng.uniform(-s, s, (n, 3)).astype(np.float32)
    xyz[:, 2] = np.abs(xyz[:, 2]) + np.float32(rng.choice([0.0, 0.5]))
    if kind == 2:
        xyz[:, 1] = xyz[0, 1]; xyz[:, 2] = xyz[0, 2]
    if kind == 3:
        xyz[:, 2] = xyz[0, 2]
    if kind == 4:
        xyz = xyz[rng.integers(0, max(1, n // 10), n)]
    rgba = rng.integers(0, 1 << 24, n).astype(np.uint32)
    if int(rng.integers(0, 3)) == 0:
        rgba[:] = rgba[0]
    pts = np.zeros((n, 4), np.float32); pts[:, :3] = xyz; pts[:, 3] = rgba.view(np.float32)
    vres = s * float(rng.choice([0.02, 0.05, 0.2]))
    prm = P.launch_params(voxel_res=vres, seed_res=vres * float(rng.choice([1, 2, 3, 8])), use_transform=int(rng.integers(0, 2)), threshold=1.0)
    truth = (np.arange(n) % 5).astype(np.uint32)
    return pts, prm, truth
