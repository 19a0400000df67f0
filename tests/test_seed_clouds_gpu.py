"""The HIP kernels of the seed stage -- d_chunkbox, d_seed_grow, d_seed_keys, d_cell_hash, d_seed_nn with its own-cell shortcut, d_seed_filter with its cell pruning,
d_seed_compact -- on the clouds of seed_clouds_common.py: every debug array, the labels and the counts of the Result against the oracle bit for bit, and SEED_ORIG and
SEED_KEPT against the brute-force reference over all voxels as well.  tests/test_seed_clouds_cpu.py shows that every case meets the condition that makes it reach its
branch, and that reference, oracle and emulation agree.

The oracle runs and the references are shared with the CPU module's (one per case and process); a case's kernel time is milliseconds, a8 (65 537 voxels, 115 sweeps) the
largest.  The narrow launches run in one child process per width, all their cases together."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import seed_clouds_common as S
from conftest import ALL_DEBUG, ROOT, first_mismatch, sha_of

pytestmark = pytest.mark.gpu

RESULT_FIELDS = ("n_points", "n_finite", "n_voxels", "octree_depth", "n_seed_cells", "n_seeds", "n_supervoxels", "n_edges", "n_merges", "n_regions", "sweeps")


def fresh(P):
    if P.device_count() < 1:
        pytest.fail("GPU test selected but libf3ds sees no HIP device (no CPU fallback exists)")
    return P.Context(0)


def assert_equals_oracle_and_reference(where, ctx, glab, r):
    gres = ctx.result
    ref = r.census.ref
    # the seed stage first, against the brute force: what differs there is the cause of whatever differs behind it
    for w, want in (("SEED_ORIG", ref.seed_orig), ("SEED_KEPT", ref.seed_kept)):
        m = S.equals(w + " (device, brute-force reference)", want, ctx.debug(w))
        assert m is None, where + ": " + m
    assert gres.n_seed_cells == r.census.C and gres.n_seeds == len(ref.seed_kept), where
    for f in RESULT_FIELDS:
        assert getattr(gres, f) == getattr(r.res, f), (where, f, getattr(gres, f), getattr(r.res, f))
    problems = [m for m in (first_mismatch(w, r.h.get(w), ctx.debug(w)) for w in ALL_DEBUG) if m]
    assert not problems, where + ":\n" + "\n".join(problems)
    assert np.array_equal(r.labels, glab), where
    assert (np.isnan(r.res.lambda_) and np.isnan(gres.lambda_)) or r.res.lambda_ == gres.lambda_, where


@pytest.mark.parametrize("name", S.NAMES)
def test_cloud_equals_the_oracle_and_the_brute_force(P, oracle, name):
    r = S.oracle_run(oracle, P, name)
    ctx = fresh(P)
    try:
        glab = ctx.segment(r.pts, r.prm)
        assert_equals_oracle_and_reference(name, ctx, glab, r)
    finally:
        ctx.close()


def test_batch_of_four_frames_equals_single_calls_and_the_oracle(P, oracle):
    """Family E: four frames of 6 to 217 seed cells in one call.  The launch of d_seed_nn / d_seed_filter is as wide as the largest frame needs: the waves of the others
    beyond their own n_cells have to return."""
    runs = [S.oracle_run(oracle, P, n) for n in S.BATCH]
    cells = [r.census.C for r in runs]
    assert max(cells) >= 16 * min(cells) and len(set(cells)) == 4, cells
    ctxs = [fresh(P) for _ in runs]
    single = fresh(P)
    try:
        got = P.segment_batch(ctxs, [r.pts for r in runs], runs[0].prm)
        for n, ctx, lab, r in zip(S.BATCH, ctxs, got, runs):
            assert ctx.launch_shape()[2] == len(runs), n
            assert_equals_oracle_and_reference("%s in a batch of %d" % (n, len(runs)), ctx, lab, r)
            slab = single.segment(r.pts, r.prm)
            assert np.array_equal(slab, lab), n
            for w in ("SEED_ORIG", "SEED_KEPT"):
                assert first_mismatch(w, single.debug(w), ctx.debug(w)) is None, n
    finally:
        single.close()
        for c in ctxs:
            c.close()


# ---- narrow launches: one child process per width -------------------------------------------------------
CHILD = (
    "import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "import conftest, seed_clouds_common as S\n"
    "P = conftest.pkg(); out = {}\n"
    "for n in %r:\n"
    "    ctx = P.Context(0)\n"
    "    lab = ctx.segment(S.frame_of(n), S.params_of(P, n))\n"
    "    out[n] = dict(shape=ctx.launch_shape(), labels=conftest.sha_of(lab), result={f: int(getattr(ctx.result, f)) for f in %r},\n"
    "                  arrays={w: conftest.sha_of(ctx.debug(w)) for w in conftest.ALL_DEBUG})\n"
    "    ctx.close()\n"
    "print(json.dumps(out))\n")


@pytest.fixture(scope="module", params=["1", "3"])
def narrow_child(request):
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), S.NARROW, RESULT_FIELDS)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, F3DS_GRID_CAP=request.param), timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return int(request.param), json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("name", S.NARROW)
def test_narrow_launch_equals_the_oracle(P, oracle, narrow_child, name):
    """A2, B5 and C1 with every launch one and three workgroups wide: the grid-stride loops of d_seed_keys, d_cell_hash and d_seed_compact go round."""
    width, out = narrow_child
    got, r = out[name], S.oracle_run(oracle, P, name)
    assert tuple(got["shape"]) == (width, width, 1), (name, got["shape"])
    for f in RESULT_FIELDS:
        assert got["result"][f] == getattr(r.res, f), (name, width, f)
    assert got["labels"] == sha_of(r.labels), (name, width)
    bad = [w for w in ALL_DEBUG if got["arrays"][w] != sha_of(r.h.get(w))]
    assert not bad, (name, width, bad)
    assert got["arrays"]["SEED_ORIG"] == sha_of(r.census.ref.seed_orig) and got["arrays"]["SEED_KEPT"] == sha_of(r.census.ref.seed_kept), (name, width)
