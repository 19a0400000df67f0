"""f3ds_refine_supervoxels -- d_refine_ghost_L, d_refine_normals, d_reseed, d_reseed_own / d_reseed_init and the sweep loop entered from a reseed -- on the clouds of
refine_clouds_common.py, against the oracle's refine bit for bit: exact ties at the reseed, within a thread's reach and across the LDS reduction, helpers that collide on one
voxel by the dozen and by the thousand, helpers erased before the reseed, ghost leaves of the seed stage alive when refine starts, iterations that run past the wrap of the
memo tag, tiles that overflowed d_normals_t's tables.  tests/test_refine_clouds_cpu.py shows that the oracle's run of each case meets the condition it is in the list for.

The oracle runs are shared with the CPU module and the vccs_clouds modules (one per case, iteration count and process).  A refine call is milliseconds of kernel time:
the 54 tests of the module take 9 s on an MI355X, 5 s of them the two child processes (test_vccs_clouds_gpu.py, its 135 tests: 10 s in the same run on the same machine).
Switches read when the library is loaded (F3DS_INC_SHIFT) and the narrow launch run in one child process per setting, all their cases together; a child returns hashes only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import refine_clouds_common as RC
from conftest import ROOT, first_mismatch, sha_of

pytestmark = pytest.mark.gpu

FULL_CASES = RC.GHOST_CASES + RC.WRAP_CASES
EXTRACT_ARRAYS = ("VOXEL_SVLABEL", "SV_CENTROID", "VOXEL_NORMAL", "VOXEL_DIST")


def fresh(P):
    if P.device_count() < 1:
        pytest.fail("GPU test selected but libf3ds sees no HIP device (no CPU fallback exists)")
    return P.Context(0)


def assert_refine_equals_oracle(where, ctx, oracle, P, name, k):
    got = ctx.refine_supervoxels(k)
    m = RC.refine_mismatch(RC.oracle_refine(oracle, P, name, k), got)
    assert m is None, "%s, refine(%d): %s" % (where, k, m)
    return got


def assert_frame_is_the_extract_state(where, ctx, r):
    """refine works on copies: the frame's own supervoxels, distances and normals are the oracle's extract arrays, and a recluster gives the oracle's labels."""
    problems = [m for m in (first_mismatch(w, r.h.get(w), ctx.debug(w)) for w in EXTRACT_ARRAYS) if m]
    assert not problems, where + ":\n" + "\n".join(problems)
    assert np.array_equal(ctx.recluster(r.prm), r.labels), where


@pytest.mark.parametrize("name", RC.NAMES)
def test_refine_equals_the_oracle_for_every_iteration_count(P, oracle, name):
    """One context: segment, then refine_supervoxels(k) for k = 0, 1, 2, 3 in that order (the every-voxel cases: as far as their oracle runs go) and k = 1 again.  All
    seven arrays equal the oracle's every time; the second k = 1 equals the first -- refine starts from the extract state each time, and the r_* copies carry nothing over
    from the longer run before it; the frame itself does not notice."""
    r = RC.oracle_run(oracle, P, name)
    ctx = fresh(P)
    try:
        assert np.array_equal(ctx.segment(r.pts, r.prm), r.labels), name
        first = None
        for k in (0,) + RC.CASE[name].ks + (1,):
            got = assert_refine_equals_oracle(name, ctx, oracle, P, name, k)
            if k == 1 and first is None:
                first = got
        assert RC.refine_mismatch(first, got) is None, name
        assert_frame_is_the_extract_state(name, ctx, r)
    finally:
        ctx.close()


def test_scratch_regrows_between_frames_of_different_sizes(P, oracle):
    """One context, frames of 65, 4914, 65, 12289, 1450 and 65 voxels (11, 64, 11, 12289, 1203 and 11 helpers), each refined: the r_* buffers and the ownR / R / stamp
    buffers the refine sweeps share with the frame's own are regrown and filled anew; what a larger frame left behind a smaller one's end is never read."""
    ctx = fresh(P)
    try:
        for name, k in (("s-chunk-straddle", 2), ("n-ring1-456-over", 2), ("s-chunk-straddle", 3), ("r-every-voxel-a-seed-12289", 1), ("g-seed-ghosts-one-sweep", 2), ("s-chunk-straddle", 2)):
            r = RC.oracle_run(oracle, P, name)
            assert np.array_equal(ctx.segment(r.pts, r.prm), r.labels), name
            assert_refine_equals_oracle("after other frames: " + name, ctx, oracle, P, name, k)
            assert_frame_is_the_extract_state("after other frames: " + name, ctx, r)
    finally:
        ctx.close()


def test_two_contexts_interleaved(P, oracle):
    """segment A, segment B, refine A, refine B, with A and B of different sizes: a context's refine reads its own frame."""
    A, B = "d-deep-chain-cold", "n-ring2-901-over"
    ra, rb = RC.oracle_run(oracle, P, A), RC.oracle_run(oracle, P, B)
    assert ra.census.V != rb.census.V and ra.census.S0 != rb.census.S0
    ca, cb = fresh(P), fresh(P)
    try:
        assert np.array_equal(ca.segment(ra.pts, ra.prm), ra.labels)
        assert np.array_equal(cb.segment(rb.pts, rb.prm), rb.labels)
        assert_refine_equals_oracle("A behind B's segment", ca, oracle, P, A, 2)
        assert_refine_equals_oracle("B behind A's refine", cb, oracle, P, B, 2)
        assert_refine_equals_oracle("A again", ca, oracle, P, A, 1)
        assert_frame_is_the_extract_state("A", ca, ra)
        assert_frame_is_the_extract_state("B", cb, rb)
    finally:
        ca.close(); cb.close()


@pytest.mark.parametrize("name", RC.GHOST_CASES)
def test_ghost_cases_on_the_global_sweep_path(P, oracle, monkeypatch, name):
    """F3DS_SWEEP_TILES = 0 (read per call): the sweeps gather globally instead of staging a tile's neighbourhood in LDS; the ghost leaves, seed-made and reseed-made, take
    that path too (the default path is the test above)."""
    monkeypatch.setenv("F3DS_SWEEP_TILES", "0")
    r = RC.oracle_run(oracle, P, name)
    ctx = fresh(P)
    try:
        assert np.array_equal(ctx.segment(r.pts, r.prm), r.labels), name
        for k in RC.CASE[name].ks:
            assert_refine_equals_oracle(name + ", global sweep path", ctx, oracle, P, name, k)
    finally:
        ctx.close()


# ---- child processes: one per switch setting, all its cases together ---------------------------------------------------------------------------------
CHILD = (
    "import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "import conftest, refine_clouds_common as RC\n"
    "P = conftest.pkg(); out = {}\n"
    "for n in %r:\n"
    "    ctx = P.Context(0)\n"
    "    lab = ctx.segment(RC.frame_of(n), RC.params_of(P, n))\n"
    "    out[n] = dict(labels=conftest.sha_of(lab), refined={})\n"
    "    for k in RC.CASE[n].ks:\n"
    "        got = ctx.refine_supervoxels(k)\n"
    "        out[n]['refined'][str(k)] = {key: [list(got[key].shape), conftest.sha_of(got[key])] for key in RC.REFINE_KEYS}\n"
    "    out[n]['shape'] = ctx.launch_shape(); out[n]['stats'] = ctx.sweep_stats()\n"
    "    ctx.close()\n"
    "print(json.dumps(out))\n")


def run_child(names, env):
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), names)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, **env), timeout=120)      # (a few seconds where it was measured)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def assert_child_equals_oracle(where, got, oracle, P, name):
    r = RC.oracle_run(oracle, P, name)
    assert got["labels"] == sha_of(r.labels), where
    assert sorted(got["refined"]) == sorted(str(k) for k in RC.CASE[name].ks), where
    for k in RC.CASE[name].ks:
        want = RC.oracle_refine(oracle, P, name, k)
        bad = [key for key in RC.REFINE_KEYS if got["refined"][str(k)][key] != [list(want[key].shape), sha_of(want[key])]]
        assert not bad, (where, k, bad)


@pytest.fixture(scope="module")
def narrow_child():
    return run_child(RC.NAMES, dict(F3DS_GRID_CAP="1"))


@pytest.fixture(scope="module")
def full_child():
    return run_child(FULL_CASES, dict(F3DS_INC_SHIFT="-1"))


@pytest.mark.parametrize("name", RC.NAMES)
def test_narrow_launch_equals_the_oracle(P, oracle, narrow_child, name):
    """Every case with every capped launch one workgroup wide (F3DS_GRID_CAP = 1): the grid-stride loops of d_refine_ghost_L, d_refine_normals, d_reseed_own and
    d_reseed_init go round -- dozens of times over the 12 289 helpers and voxels of the largest case."""
    got = narrow_child[name]
    assert tuple(got["shape"]) == (1, 1, 1), name
    assert_child_equals_oracle(name + " at width 1", got, oracle, P, name)


@pytest.mark.parametrize("name", FULL_CASES)
def test_every_sweep_full_equals_the_oracle(P, oracle, full_child, name):
    """The ghost and wrap cases with every sweep full (F3DS_INC_SHIFT = -1, read when the library is loaded): the memoised walker runs in every busy sweep of every
    iteration, past the wrap of its tag, and over the ghost leaves the reseed made."""
    got = full_child[name]
    sweeps = RC.oracle_run(oracle, P, name).census.sweeps
    if sweeps:      # the statistics are those of the last run of sweeps, the last iteration's: all its sweeps counted, none incremental, none a fallback
        assert sum(got["stats"]) == sweeps and got["stats"][1] == 0 and got["stats"][2] == 0, (name, got["stats"])
    assert_child_equals_oracle(name + " with every sweep full", got, oracle, P, name)
