"""Scoring over a sparse contingency table (csrc/f3ds_eval_levels.h), without a GPU: a g++ harness runs the shared routine -- visiting
order, matching, the seven ordered sums -- on seeded random tables and on hand-made ones with every quirk of the reference's matching, and
compares it with f3ds_scores_from_table (csrc/f3ds_eval.h, the dense scoring of f3ds_evaluate) on the dense form of the same table."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HARNESS_SRC = os.path.join(ROOT, "tests", "eval_levels_harness", "eval_levels_harness.cpp")
FIELDS = ("voi", "precision", "recall", "fscore", "wov", "fpr", "fnr")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("eval_levels_harness") / "libeval_levels_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, HARNESS_SRC], check=True)
    lib = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    lib.evl_check.argtypes = [ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint32, vp]
    lib.evl_check.restype = None
    return lib


def _run(lib, table, ssize, tsize, N):
    table = np.ascontiguousarray(table, np.uint32)
    K, M = table.shape
    ssize = np.ascontiguousarray(ssize, np.uint32)
    tsize = np.ascontiguousarray(tsize, np.uint32)
    out = np.zeros(21, np.float32)
    lib.evl_check(K, M, table.ctypes.data, ssize.ctypes.data, tsize.ctypes.data, int(N), out.ctypes.data)
    return out[:7], out[7:14], out[14:]


def _check(lib, table, ssize, tsize, N, what):
    dense, sparse_std, sparse_m = _run(lib, table, ssize, tsize, N)
    assert np.all(np.isfinite(dense)), what
    assert dense.view(np.uint32).tolist() == sparse_std.view(np.uint32).tolist(), \
        "%s: std::log instance differs: %s vs %s" % (what, dict(zip(FIELDS, dense)), dict(zip(FIELDS, sparse_std)))
    assert dense[1:].view(np.uint32).tolist() == sparse_m[1:].view(np.uint32).tolist(), "%s: m_logf instance, log-free fields" % what
    assert abs(float(dense[0]) - float(sparse_m[0])) <= 1e-5, "%s: voi %r vs %r" % (what, dense[0], sparse_m[0])
    return dense


def _matching(table, tsize):
    """The plain reading of Testing's matching (testing.cpp:88-136) on a dense table, for the quirk bookkeeping of the tests below:
    returns (match per label, notes) where notes holds the quirks the table exercised."""
    K, M = table.shape
    by_size = {}
    for j in range(M):
        by_size.setdefault(int(tsize[j]), j)
    used = np.zeros(K, bool)
    match = [-1] * M
    notes = set()
    if len(by_size) < M:
        notes.add("equal sizes")
    for size in sorted(by_size, reverse=True):
        j = by_size[size]
        col = table[:, j].astype(np.int64).copy()
        if not col.any():
            notes.add("empty column, row 0 used" if used[0] else "empty column, row 0 free")
        nz = col[col > 0]
        if len(nz) and len(set(nz.tolist())) < len(nz):
            notes.add("equal counts")
        row = -1
        while True:
            best = int(np.argmax(col))
            if not used[best]:
                row = best
                break
            col[best] = 0
            if not col.any():
                break
        match[j] = row
        if row >= 0:
            used[row] = True
    return match, notes


def _random_case(rng, K, M, density, extra_n):
    table = np.where(rng.random((K, M)) < density, rng.integers(1, 6, (K, M)), 0).astype(np.uint32)
    empty_cols = rng.choice(M, max(1, M // 6), replace=False) if M > 1 else []
    table[:, empty_cols] = 0
    ssize = table.sum(1).astype(np.uint32) + rng.integers(0, 3, K).astype(np.uint32)       # (ghost leaves: size without intersection)
    ssize[ssize == 0] = 1
    tsize = table.sum(0).astype(np.uint32) + rng.integers(0, 4, M).astype(np.uint32)       # (voxels outside every segment)
    tsize[tsize == 0] = 1
    if M >= 4:                                                                               # equal truth sizes
        a, b = rng.choice(M, 2, replace=False)
        tsize[b] = max(tsize[a], table[:, b].sum())
        tsize[a] = tsize[b]
    N = int(tsize.sum()) + extra_n
    return table, ssize, tsize, N


def test_random_tables_match_dense_scoring(harness):
    rng = np.random.default_rng(20261016)
    seen = set()
    for it in range(400):
        K = int(rng.integers(1, 40))
        M = int(rng.integers(1, 40))
        table, ssize, tsize, N = _random_case(rng, K, M, float(rng.uniform(0.05, 0.6)), int(rng.choice([0, 5, 100000])))
        _check(harness, table, ssize, tsize, N, "case %d (K %d, M %d)" % (it, K, M))
        seen |= _matching(table, tsize)[1]
    assert seen >= {"equal sizes", "empty column, row 0 free", "empty column, row 0 used", "equal counts"}, seen


def test_many_truth_labels(harness):
    # thousands of labels, many of equal size: the visiting order is O(M^2) (flags once, then ranks), so this takes milliseconds
    rng = np.random.default_rng(11)
    table, ssize, tsize, N = _random_case(rng, 60, 3000, 0.01, 1000)
    tsize[rng.choice(3000, 1500, replace=False)] = tsize[0]
    tsize = np.maximum(tsize, table.sum(0)).astype(np.uint32)
    N = int(tsize.sum()) + 1000
    _check(harness, table, ssize, tsize, N, "K 60, M 3000")
    assert len(set(tsize.tolist())) < 3000


def test_one_row_and_one_column(harness):
    rng = np.random.default_rng(7)
    for it in range(50):
        M = int(rng.integers(1, 12))
        table, ssize, tsize, N = _random_case(rng, 1, M, 0.5, int(rng.integers(0, 50)))
        _check(harness, table, ssize, tsize, N, "K = 1, case %d" % it)
        K = int(rng.integers(1, 12))
        table, ssize, tsize, N = _random_case(rng, K, 1, 0.5, int(rng.integers(0, 50)))
        _check(harness, table, ssize, tsize, N, "M = 1, case %d" % it)
    # a single cell, and a single empty cell (the all-zero truth of a frame whose voxels are all unowned)
    _check(harness, [[3]], [3], [3], 3, "1 x 1")
    _check(harness, [[0]], [2], [5], 5, "1 x 1 empty")


def test_hand_made_quirks(harness):
    # labels 0 and 1 have size 6: only label 0 is visited (std::map keeps the first label of a size), and it takes row 1 (counts 3, 3:
    # the lower row); label 1 stays unmatched; label 2's column is empty and row 0 is still free: it takes row 0 with an intersection of 0
    table = np.array([[0, 2, 0], [3, 4, 0], [3, 0, 0]], np.uint32)
    ssize, tsize = [3, 7, 3], [6, 6, 2]
    match, notes = _matching(table, tsize)
    assert match == [1, -1, 0] and {"equal sizes", "empty column, row 0 free", "equal counts"} <= notes
    _check(harness, table, ssize, tsize, 20, "equal sizes + empty column")
    # equal counts in a column: the lower row wins; then an empty column finds row 0 used and stays unmatched
    table = np.array([[5, 0], [5, 0], [1, 0]], np.uint32)
    ssize, tsize = [5, 6, 1], [11, 1]
    match, notes = _matching(table, tsize)
    assert match == [0, -1] and {"equal counts", "empty column, row 0 used"} <= notes
    _check(harness, table, ssize, tsize, 12, "equal counts + row 0 used")
    # every row of a column already used: unmatched
    table = np.array([[4, 1], [0, 0]], np.uint32)
    match, _ = _matching(table, [4, 3])
    assert match == [0, -1]
    _check(harness, table, [5, 2], [4, 3], 9, "column of used rows")
    # N far above the table mass
    _check(harness, table, [5, 2], [4, 3], 10 ** 7, "large N")
