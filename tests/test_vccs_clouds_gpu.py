"""The HIP kernels of the supervoxel half -- voxelisation on either path, neighbour search, d_normals_t with its LDS tables and its global-memory fallback, seeds, the
label-propagation sweeps (full, incremental, idle, past the wrap of the memo tag, with chains deeper than the walkers' stack), d_centroid / d_sv_fill on both sides of
their row path, the relabel on both sides of its LDS table -- on the synthetic lattice clouds of vccs_clouds_common.py, against the oracle bit for bit: labels, the counts
of the Result and every debug array.  tests/test_vccs_clouds_cpu.py shows that the oracle's run of each case meets the condition that makes it exercise its path.

The oracle and emulation runs are shared with the CPU module's (one per case and process; 1.4 s of oracle time for all 50 cases); a case's kernel time is milliseconds:
the 139 tests of the module take 11 s on an MI355X, 5 s of them the two child processes.
Switches read when the library is loaded (F3DS_INC_SHIFT) and the narrow launch run in one child process per setting, all their cases together."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import vccs_clouds_common as C
from conftest import ALL_DEBUG, ROOT, first_mismatch, sha_of

pytestmark = pytest.mark.gpu

RESULT_FIELDS = ("n_points", "n_finite", "n_voxels", "octree_depth", "n_seed_cells", "n_seeds", "n_supervoxels", "n_edges", "n_merges", "n_regions", "sweeps")
FAMILY_1 = [c.name for c in C.CASES if c.family == 1]
SWEEP_CASES = [c.name for c in C.CASES if c.family in (4, 5)] + ["r-tiny-supervoxels-desc", "r-big-supervoxels", "v-desc-big-supervoxels"]
FULL_CASES = [c.name for c in C.CASES if c.also_full]
NARROW_CASES = [c.name for c in C.CASES if c.family in (1, 3, 4)]
BATCH_FAMILIES = (1, 3, 4)


TILE_TRACE = re.compile(r"tile path: most voxels in a tile (\d+), descriptors \d+, leaves (\d+), lists sorted (\d+)")


def fresh(P):
    if P.device_count() < 1:
        pytest.fail("GPU test selected but libf3ds sees no HIP device (no CPU fallback exists)")
    return P.Context(0)


def assert_equals_oracle(where, ctx, glab, r):
    """Labels, the counts of the Result, lambda and every array of ALL_DEBUG against the oracle's run r."""
    gres = ctx.result
    for f in RESULT_FIELDS:
        assert getattr(gres, f) == getattr(r.res, f), (where, f, getattr(gres, f), getattr(r.res, f))
    problems = [m for m in (first_mismatch(w, r.h.get(w), ctx.debug(w)) for w in ALL_DEBUG) if m]
    assert not problems, where + ":\n" + "\n".join(problems)
    assert np.array_equal(r.labels, glab), where
    assert (np.isnan(r.res.lambda_) and np.isnan(gres.lambda_)) or r.res.lambda_ == gres.lambda_, where


@pytest.mark.parametrize("name", C.NAMES)
def test_cloud_equals_the_oracle_on_either_stage0_path(P, oracle, monkeypatch, capfd, name):
    """As a lone call gets it (the sort path), with the sort path asked for, and with the tile path forced -- twice on that context: a frame the tile path refuses (a
    voxel of more than 256 points, a tile of more than 1280 voxels) runs again on the sort path in the same call, and the context remembers.  What the tile kernels
    themselves counted (F3DS_TRACE_ERR, read per call) is the census's: the most voxels of a tile, whether vox_disorder was set (the leaf lists are then sorted in place),
    and why a frame was refused."""
    r = C.oracle_run(oracle, P, name)
    want_path = C.predicted_stage0(r.census, r.res.octree_depth)
    ctx = fresh(P)
    try:
        for env in (None, "0"):
            if env is None:
                monkeypatch.delenv("F3DS_VOX_TILES", raising=False)
            else:
                monkeypatch.setenv("F3DS_VOX_TILES", env)
            glab = ctx.segment(r.pts, r.prm)
            assert ctx.stage0_path() == "sort", (name, env)
            assert_equals_oracle("%s, F3DS_VOX_TILES %s" % (name, env), ctx, glab, r)
    finally:
        ctx.close()
    monkeypatch.setenv("F3DS_VOX_TILES", "2")
    monkeypatch.setenv("F3DS_TRACE_ERR", "1")
    ctx = fresh(P)
    try:
        for call in (1, 2):
            capfd.readouterr()
            glab = ctx.segment(r.pts, r.prm)
            err = capfd.readouterr().err
            assert ctx.stage0_path() == want_path, (name, call, r.census.max_points_per_voxel, r.census.max_tile_voxels)
            counted = TILE_TRACE.findall(err)
            if want_path == "tiles":
                assert counted == [(str(r.census.max_tile_voxels), str(r.census.V), str(int(r.census.disorder)))] and "refused" not in err, (name, call, err)
            elif call == 1:
                why = "a voxel with too many points" if r.census.max_points_per_voxel > C.VL_MAX_RUN else "a tile with too many voxels"
                assert len(counted) == 1 and "tile path refused a frame: " + why in err, (name, err)
            else:
                assert counted == [], (name, err)      # (the context went straight to the sort path)
            assert_equals_oracle("%s, tile path forced, call %d" % (name, call), ctx, glab, r)
    finally:
        ctx.close()


@pytest.mark.parametrize("threads", [None, "256", "384"])
@pytest.mark.parametrize("name", FAMILY_1)
def test_normals_tables_overflow_where_the_census_says(P, oracle, monkeypatch, name, threads):
    """d_normals_t<384> and <256>: the one-ring list of every tile that fits is as long as the census counts it, and exactly the tiles whose one-ring exceeds 448 or whose
    two-ring exceeds 896 read 0xFFFFFFFF (one_tile sets tile_n1 = SW_TILE_NONE for either kind of overflow; the tile's normals then come from the global-memory
    accumulation and the sweeps gather globally there).  Normals, and what the sweeps make of the tables, against the oracle."""
    if threads is None:
        monkeypatch.delenv("F3DS_NORMALS_THREADS", raising=False)
    else:
        monkeypatch.setenv("F3DS_NORMALS_THREADS", threads)
    r = C.oracle_run(oracle, P, name)
    ctx = fresh(P)
    try:
        glab = ctx.segment(r.pts, r.prm)
        tl = ctx.tile_list_lengths()
        cen = r.census
        assert len(tl) == len(cen.ring1)
        assert np.array_equal(tl == C.TILE_NONE, cen.overflow), (name, np.nonzero((tl == C.TILE_NONE) != cen.overflow)[0][:8])
        assert np.array_equal(tl[cen.fits], cen.ring1[cen.fits].astype(np.uint32)), name
        assert_equals_oracle("%s, F3DS_NORMALS_THREADS %s" % (name, threads), ctx, glab, r)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", SWEEP_CASES)
def test_sweep_statistics_equal_the_emulation(P, oracle, emul, name):
    r = C.oracle_run(oracle, P, name)
    er = C.emul_run_of(emul, P, name)
    ctx = fresh(P)
    try:
        glab = ctx.segment(r.pts, r.prm)
        assert ctx.sweep_stats() == er.stats and sum(er.stats) == ctx.result.sweeps, (name, ctx.sweep_stats(), er.stats)
        assert np.array_equal(glab, r.labels)
    finally:
        ctx.close()


# ---- child processes: one per switch setting, all its cases together ---------------------------------------------------------------------------------
CHILD = (
    "import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "import conftest, vccs_clouds_common as C\n"
    "P = conftest.pkg(); out = {}\n"
    "for n in %r:\n"
    "    ctx = P.Context(0)\n"
    "    lab = ctx.segment(C.frame_of(n), C.params_of(P, n))\n"
    "    out[n] = dict(shape=ctx.launch_shape(), labels=conftest.sha_of(lab), stats=ctx.sweep_stats(), result={f: int(getattr(ctx.result, f)) for f in %r},\n"
    "                  arrays={w: conftest.sha_of(ctx.debug(w)) for w in conftest.ALL_DEBUG})\n"
    "    ctx.close()\n"
    "print(json.dumps(out))\n")


def run_child(names, env):
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), names, RESULT_FIELDS)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, **env), timeout=120)      # (about 3 s where it was measured)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def assert_child_equals_oracle(where, got, r):
    for f in RESULT_FIELDS:
        assert got["result"][f] == getattr(r.res, f), (where, f)
    assert got["labels"] == sha_of(r.labels), where
    bad = [w for w in ALL_DEBUG if got["arrays"][w] != sha_of(r.h.get(w))]
    assert not bad, (where, bad)


@pytest.fixture(scope="module")
def narrow_child():
    return run_child(NARROW_CASES, dict(F3DS_GRID_CAP="1"))


@pytest.fixture(scope="module")
def full_child():
    return run_child(FULL_CASES, dict(F3DS_INC_SHIFT="-1"))


@pytest.mark.parametrize("name", NARROW_CASES)
def test_narrow_launch_equals_the_oracle(P, oracle, narrow_child, name):
    """Families 1, 3 and 4 with every launch one workgroup wide (F3DS_GRID_CAP = 1): every grid-stride loop goes round."""
    got = narrow_child[name]
    assert tuple(got["shape"]) == (1, 1, 1), name
    assert_child_equals_oracle(name + " at width 1", got, C.oracle_run(oracle, P, name))


@pytest.mark.parametrize("name", FULL_CASES)
def test_every_sweep_full_equals_the_oracle_and_the_emulation(P, oracle, emul, full_child, name):
    """The long runs with every sweep full (F3DS_INC_SHIFT = -1, read when the library is loaded): the memoised walker runs in sweeps 63, 64, ... and 126, 127, ...,
    where the tag has wrapped."""
    got = full_child[name]
    r = C.oracle_run(oracle, P, name)
    er = C.emul_run_of(emul, P, name, "-1")
    assert tuple(got["stats"]) == er.stats and got["stats"][C.INCREMENTAL] == 0 and got["stats"][C.FALLBACK] == 0, (name, got["stats"], er.stats)
    assert_child_equals_oracle(name + " with every sweep full", got, r)


# ---- batches ---------------------------------------------------------------------------------------------------------------------------------------
def _batch_groups(family):
    """The cases of a family, grouped by their parameters (a batch call takes one set)."""
    groups = {}
    for c in C.CASES:
        if c.family == family:
            groups.setdefault(tuple(sorted(c.params.items())), []).append(c.name)
    return list(groups.values())


@pytest.mark.parametrize("family", BATCH_FAMILIES)
def test_family_as_batches_equals_the_oracle(P, oracle, monkeypatch, family):
    """All cases of a family through segment_batch, one call per set of parameters: a frame's share of the launch is narrower, tiles that overflow and tiles that fit of
    several frames share one launch of d_normals_t<384>, and runs of 8, 71 and 128 sweeps share one sweep loop."""
    monkeypatch.delenv("F3DS_VOX_TILES", raising=False)
    groups = _batch_groups(family)
    assert sum(len(g) for g in groups) == len([c for c in C.CASES if c.family == family])
    for names in groups:
        runs = [C.oracle_run(oracle, P, n) for n in names]
        ctxs = [fresh(P) for _ in names]
        try:
            got = P.segment_batch(ctxs, [r.pts for r in runs], runs[0].prm)
            for n, ctx, lab, r in zip(names, ctxs, got, runs):
                assert ctx.launch_shape()[2] == len(names), n
                assert_equals_oracle("%s in a batch of %d" % (n, len(names)), ctx, lab, r)
        finally:
            for c in ctxs:
                c.close()
