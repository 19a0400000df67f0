"""Parity under narrow launches.  Production runs 192 frames per batch call, which leaves a frame 16 workgroups: every grid-stride loop of
csrc/f3ds_kernels.inc goes round many times there, while a lone golden frame at its default width (2048 workgroups) is done in one trip.  Here the
development switch F3DS_GRID_CAP narrows every launch to 1, 3 or 8 workgroups per frame, so that the loops make their second and later trips -- LDS tiles
staged again, ballots and block scans with lanes that have run out of work, ragged last trips -- on frames the oracle finishes in a second, and every
intermediate array is compared with the oracle and the committed hashes, bit for bit.  Context.launch_shape() is asserted first in every test: equal
hashes alone would not show that the narrow launch was in force.  tests/test_narrow_launch_cpu.py shows that the cases and widths used here reach
every family of loops (narrow_launch_common.FAMILIES)."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ALL_DEBUG, ROOT, first_mismatch, same_bits, sha_of
from golden_cases import case_params, case_points, synthetic_truth
from narrow_launch_common import (BATCH_SIZES, BATCH_WIDTHS, ENTRY_CASES, ENTRY_WIDTHS, LEVEL_CASES, LEVEL_WIDTHS, SINGLE_CASES, STAGE0, SWEEP_VARIANT_ARRAYS,
                                  SWEEP_VARIANT_CASES, SWEEP_VARIANT_WIDTH, SWEEP_VARIANTS, TILE_PATH_REFUSES)
from test_eval_levels_gpu import check_golden_level_scores, harness  # noqa: F401  (harness: the module-scoped fixture of the level-score tests)
from test_levels_gpu import check_golden_levels

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_golden.json")))
RESULT_FIELDS = ("n_points", "n_finite", "n_voxels", "octree_depth", "n_seed_cells", "n_seeds", "n_supervoxels", "n_edges", "n_merges", "n_regions", "sweeps")


class OracleRuns:
    """One oracle run per distinct (frame, parameters), shared by the tests of the module."""

    def __init__(self, oracle):
        self.oracle, self.runs = oracle, {}

    def segment(self, pts, prm):
        key = hashlib.sha256(np.ascontiguousarray(pts).tobytes() + bytes(ctypes.string_at(ctypes.addressof(prm), ctypes.sizeof(prm)))).hexdigest()
        if key not in self.runs:
            self.runs[key] = self.oracle.segment(pts, prm)
            assert self.runs[key][0] == 0
        return self.runs[key]

    def case(self, P, name):
        return self.segment(case_points(P, name), case_params(P, name))


@pytest.fixture(scope="module")
def oracle_runs(oracle):
    return OracleRuns(oracle)


@pytest.fixture(scope="module")
def level_oracle_runs(oracle):
    """Runs of their own for the level tests, which call cluster(t) on them: the runs above stay as segment() left them."""
    return OracleRuns(oracle)


@pytest.fixture
def fresh_ctx(P):
    """A context without a past: one that met a frame the tile path refuses sends its next frames down the sort path whatever F3DS_VOX_TILES says."""
    ctx = P.Context(0)
    yield ctx
    ctx.close()


def narrow(monkeypatch, width):
    monkeypatch.setenv("F3DS_GRID_CAP", str(width))


def assert_every_array(name, ctx, glab, olab, ores, oh, gold=None):
    """The body of test_every_stage_matches_oracle_and_golden: result fields, the 20 debug arrays, labels, lambda, the voxel cloud."""
    gres = ctx.result
    for f in RESULT_FIELDS:
        assert getattr(gres, f) == getattr(ores, f), (name, f)
    problems = []
    for what in ALL_DEBUG:
        got = ctx.debug(what)
        m = first_mismatch(what, oh.get(what), got)
        if m:
            problems.append(m)
        elif gold is not None:
            assert sha_of(got) == gold["sha256"][what], (name, what)
    assert not problems, name + ":\n" + "\n".join(problems)
    assert np.array_equal(olab, glab), name
    if gold is not None:
        assert sha_of(glab) == gold["labels_sha256"], name
    assert (np.isnan(ores.lambda_) and np.isnan(gres.lambda_)) or ores.lambda_ == gres.lambda_, name
    ox, ol, oc = oh.voxel_cloud()
    gx, gl, gc = ctx.voxel_cloud()
    assert np.array_equal(ox.view(np.uint32), gx.view(np.uint32)) and np.array_equal(ol, gl) and np.array_equal(oc, gc), name


# ---- a. single frames -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stage0", STAGE0)
@pytest.mark.parametrize("name,width", [(n, w) for n, widths in SINGLE_CASES for w in widths])
def test_single_frame_every_stage_matches_oracle_and_golden(P, oracle_runs, fresh_ctx, monkeypatch, name, width, stage0):
    narrow(monkeypatch, width)
    monkeypatch.setenv("F3DS_VOX_TILES", "2" if stage0 == "tiles" else "0")
    pts, prm = case_points(P, name), case_params(P, name)
    glab = fresh_ctx.segment(pts, prm)
    assert fresh_ctx.launch_shape() == (width, width, 1)
    assert fresh_ctx.stage0_path() == ("sort" if name in TILE_PATH_REFUSES else stage0)      # (a refused frame has run the tile kernels and then the sort path)
    _, olab, ores, oh = oracle_runs.case(P, name)
    assert_every_array(name, fresh_ctx, glab, olab, ores, oh, GOLD[name])


def test_launch_shape_without_the_switch(P, gpu_ctx, monkeypatch):
    """Unset (or out of range, or without F3DS_DEV) the switch moves nothing: a lone frame gets 2048 workgroups from both caps, a frame of a batch of 16 its
    share of 3072 from grid_for()."""
    monkeypatch.delenv("F3DS_GRID_CAP", raising=False)
    pts, prm = case_points(P, "rgbd_160x120"), case_params(P, "rgbd_160x120")
    gpu_ctx.segment(pts, prm)
    assert gpu_ctx.launch_shape() == (2048, 2048, 1)
    for bad in ("0", "2049", "-3", "x"):
        monkeypatch.setenv("F3DS_GRID_CAP", bad)
        gpu_ctx.segment(pts, prm)
        assert gpu_ctx.launch_shape() == (2048, 2048, 1), bad
    monkeypatch.delenv("F3DS_GRID_CAP")
    ctxs = [P.Context(0) for _ in range(16)]
    try:
        P.segment_batch(ctxs, [pts] * 16, prm)
        assert [c.launch_shape() for c in ctxs] == [(192, 2048, 16)] * 16
        monkeypatch.setenv("F3DS_GRID_CAP", "2048")
        P.segment_batch(ctxs, [pts] * 16, prm)
        assert [c.launch_shape() for c in ctxs] == [(2048, 2048, 16)] * 16
    finally:
        for c in ctxs:
            c.close()


# ---- b. sweep variants (F3DS_INC_SHIFT is read when the library is loaded: a child process per variant) ---------------------------------------------

@pytest.mark.parametrize("variant", SWEEP_VARIANTS, ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()))
def test_sweep_variants_match_the_golden_hashes(variant):
    code = (
        "import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import conftest; from golden_cases import case_points, case_params\n"
        "P = conftest.pkg(); ctx = P.Context(0); out = {}\n"
        "for n in %r:\n"
        "    lab = ctx.segment(case_points(P, n), case_params(P, n))\n"
        "    out[n] = dict(shape=ctx.launch_shape(), labels=conftest.sha_of(lab), stats=ctx.sweep_stats(), sweeps=int(ctx.result.sweeps), **{w: conftest.sha_of(ctx.debug(w)) for w in %r})\n"
        "print(json.dumps(out))\n") % (ROOT, os.path.join(ROOT, "tests"), SWEEP_VARIANT_CASES, SWEEP_VARIANT_ARRAYS)
    env = dict(os.environ, F3DS_GRID_CAP=str(SWEEP_VARIANT_WIDTH), **variant)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for n in SWEEP_VARIANT_CASES:
        assert tuple(got[n]["shape"]) == (SWEEP_VARIANT_WIDTH, SWEEP_VARIANT_WIDTH, 1), (n, variant)
        assert got[n]["labels"] == GOLD[n]["labels_sha256"], (n, variant)
        for w in SWEEP_VARIANT_ARRAYS:
            assert got[n][w] == GOLD[n]["sha256"][w], (n, w, variant)
        assert sum(got[n]["stats"]) == got[n]["sweeps"] == GOLD[n]["summary"]["sweeps"], (n, variant, got[n]["stats"])
        if variant.get("F3DS_INC_SHIFT") == "-1":
            assert got[n]["stats"][1] == 0 and got[n]["stats"][2] == 0, (n, got[n]["stats"])      # no sweep is incremental
        if variant.get("F3DS_INC_SHIFT") == "32":
            assert got[n]["stats"][1] + got[n]["stats"][2] > 0, (n, got[n]["stats"])               # ... some are
        if "F3DS_R_ROUNDS_RUN" in variant:
            assert got[n]["stats"][2] > 0, (n, got[n]["stats"])                                    # the whole-grid fallback loop of d_sweep_R ran


# ---- c. the other entry points ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def entry_refs(P, oracle):
    """Per case, from one oracle run of its own (cluster() moves that run's state: it comes last): evaluate, refine(2), and a recluster with other merge settings."""
    refs = {}
    for name in ENTRY_CASES:
        pts, prm = case_points(P, name), case_params(P, name)
        rc, olab, ores, oh = oracle.segment(pts, prm)
        assert rc == 0
        truth = synthetic_truth(pts)
        rc, perf = oh.evaluate(truth)
        assert rc == 0
        refined = oh.refine(2)
        cloud = oh.voxel_cloud()
        prm2 = prm.copy(); prm2.threshold = 0.12; prm2.color_metric = P.RGB_EUCL
        rc, lab2, res2 = oh.cluster(prm2, len(pts))
        assert rc == 0
        cloud2 = oh.voxel_cloud()
        refs[name] = dict(pts=pts, prm=prm, truth=truth, labels=olab, perf=perf.as_dict(), refined=refined, cloud=cloud, prm2=prm2, labels2=lab2,
                          regions2=int(res2.n_regions), merges2=int(res2.n_merges), cloud2=cloud2)
    return refs


def _segment_narrow(ctx, ref, monkeypatch, width):
    narrow(monkeypatch, width)
    glab = ctx.segment(ref["pts"], ref["prm"])
    assert ctx.launch_shape() == (width, width, 1)
    assert np.array_equal(glab, ref["labels"])


def _same_cloud(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("width", ENTRY_WIDTHS)
@pytest.mark.parametrize("name", ENTRY_CASES)
def test_recluster_and_voxel_cloud(P, entry_refs, gpu_ctx, monkeypatch, name, width):
    ref = entry_refs[name]
    _segment_narrow(gpu_ctx, ref, monkeypatch, width)
    assert _same_cloud(ref["cloud"], gpu_ctx.voxel_cloud())
    other = 4 - width                                     # the width of this call, not the one the frame was segmented at
    narrow(monkeypatch, other)
    lab2 = gpu_ctx.recluster(ref["prm2"])
    assert gpu_ctx.launch_shape() == (other, other, 1)
    assert np.array_equal(lab2, ref["labels2"])
    assert (gpu_ctx.result.n_regions, gpu_ctx.result.n_merges) == (ref["regions2"], ref["merges2"])
    assert _same_cloud(ref["cloud2"], gpu_ctx.voxel_cloud())


@pytest.mark.parametrize("width", ENTRY_WIDTHS)
@pytest.mark.parametrize("name", ENTRY_CASES)
def test_evaluate(P, entry_refs, gpu_ctx, monkeypatch, name, width):
    ref = entry_refs[name]
    _segment_narrow(gpu_ctx, ref, monkeypatch, 4 - width)
    narrow(monkeypatch, width)                            # f3ds_evaluate reads the switches itself
    perf = gpu_ctx.evaluate(ref["truth"])
    assert gpu_ctx.launch_shape() == (width, width, 1)
    assert perf.as_dict() == ref["perf"]


@pytest.mark.parametrize("width", ENTRY_WIDTHS)
@pytest.mark.parametrize("name", ENTRY_CASES)
def test_refine_supervoxels(P, entry_refs, gpu_ctx, monkeypatch, name, width):
    ref = entry_refs[name]
    _segment_narrow(gpu_ctx, ref, monkeypatch, width)
    got = gpu_ctx.refine_supervoxels(2)
    assert gpu_ctx.launch_shape() == (width, width, 1)
    want = ref["refined"]
    for key in ("voxel_label", "label", "n_voxels", "voxel_normal", "xyz", "rgb", "normal"):
        assert want[key].shape == got[key].shape, key
        assert same_bits(want[key], got[key]), (key, first_mismatch(key, want[key], got[key]))
    assert np.array_equal(gpu_ctx.recluster(ref["prm"]), ref["labels"])      # the frame's own state did not notice


# ---- d. batches: full groups of eight frames and a remainder (f3ds_vblock) --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def batch_frames(P, oracle_runs):
    """17 distinct frames (a batch of 9 takes the first nine): 160x120 frames of different seeds, an empty frame and a 320x240 one among the first nine."""
    prm = P.launch_params(voxel_res=0.03, seed_res=0.3)      # (~500 voxels per 4096 points: the tile path, which a batch takes, accepts every frame)
    frames = [P.synth_frame(0, 4200 + i, 160, 120, 30) for i in range(max(BATCH_SIZES))]
    frames[3] = np.zeros((0, 4), np.float32)
    frames[6] = P.synth_frame(0, 4300, 320, 240, 40)
    assert len({f.tobytes() for f in frames}) == len(frames)
    return prm, frames, [oracle_runs.segment(f, prm) for f in frames]


@pytest.mark.parametrize("width", BATCH_WIDTHS)
@pytest.mark.parametrize("nf", BATCH_SIZES)
def test_batch_with_a_remainder_frame(P, batch_frames, monkeypatch, nf, width):
    prm, frames, runs = batch_frames
    narrow(monkeypatch, width)
    ctxs = [P.Context(0) for _ in range(nf)]
    try:
        got = P.segment_batch(ctxs, frames[:nf], prm)
        assert [c.launch_shape() for c in ctxs] == [(width, width, nf)] * nf
        for i in range(nf):
            _, olab, ores, oh = runs[i]
            if len(frames[i]) == 0:                       # the empty frame has no arrays: its (empty) labels and counts
                assert len(got[i]) == 0 and ctxs[i].result.n_regions == ores.n_regions == 0
                continue
            assert ctxs[i].stage0_path() == "tiles", i    # (what the frames of a batch take)
            assert_every_array("frame %d of %d" % (i, nf), ctxs[i], got[i], olab, ores, oh)
    finally:
        for c in ctxs:
            c.close()


# ---- e. hierarchy levels and their scores -----------------------------------------------------------------------------------------------------------

def _shape_is(width):
    def check(ctx):
        assert ctx.launch_shape() == (width, width, 1)
    return check


@pytest.mark.parametrize("width", LEVEL_WIDTHS)
@pytest.mark.parametrize("name", LEVEL_CASES)
def test_levels_equal_recluster_and_oracle(P, level_oracle_runs, gpu_ctx, monkeypatch, name, width):
    narrow(monkeypatch, width)
    check_golden_levels(P, level_oracle_runs, gpu_ctx, monkeypatch, name, after_segment=_shape_is(width))


@pytest.mark.parametrize("width", LEVEL_WIDTHS)
@pytest.mark.parametrize("name", LEVEL_CASES)
def test_level_scores_equal_recluster_evaluate_and_the_host_build(P, gpu_ctx, harness, monkeypatch, name, width):  # noqa: F811
    narrow(monkeypatch, width)
    check_golden_level_scores(P, gpu_ctx, harness, name, after_call=_shape_is(width))
