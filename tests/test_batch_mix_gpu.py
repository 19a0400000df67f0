"""segment_batch on batches whose frames disagree on every decision the host takes for the whole batch (batch_mix_common.py): every frame of every mix against the
oracle's lone run of that frame bit for bit -- labels, the counts of the Result and every debug array -- and, per mix, what the call has to show: stage0_path(),
merge_layout(), launch_shape() and the F3DS_TRACE_ERR lines on stderr.  tests/test_batch_mix_cpu.py shows that the oracle's runs meet the condition of every mix.

What a test predicts comes from the oracle's runs and the formulas of batch_mix_common.py, never from the device's answer.  The oracle runs are shared with the CPU
module's (one per frame and parameter set and process; block(24, 24, 24) takes 4 s of oracle time, everything else a second together); a mix's kernel time is
milliseconds: the 21 tests of the module take 6.5 s on an MI355X, 3.8 s of them that one oracle run."""
import re

import numpy as np
import pytest

import batch_mix_common as B
from conftest import first_mismatch
from test_vccs_clouds_gpu import RESULT_FIELDS, assert_equals_oracle, fresh

pytestmark = pytest.mark.gpu

REFUSED = "tile path refused a frame"
REFUSED_WHY = "tile path refused a frame: a voxel with too many points"
VOX_AGAIN = re.compile(r"voxelisation of (\d+) frames runs again on the sort path")
ADJ_AGAIN = re.compile(r"adjacency pass of (\d+) frames runs again with more list room")
MERGE_AGAIN = re.compile(r"merge stage of (\d+) frames runs again with more history / leaf-pool room")
MERGE_GLOBAL_AGAIN = "runs again with the global-memory kernel"


def set_env(monkeypatch, env):
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def contexts(P, n):
    return [fresh(P) for _ in range(n)]


def close_all(ctxs):
    for c in ctxs:
        c.close()


def run_batch(P, ctxs, runs):
    return P.segment_batch(ctxs, [r.pts for r in runs], runs[0].prm)


def assert_dead(where, P, ctx, lab, r):
    """A frame that left the batch: every label F3DS_NO_LABEL, the counts the oracle's."""
    assert r.res.n_voxels == 0 and len(lab) == len(r.pts) and (lab == P.NO_LABEL).all() and np.array_equal(lab, r.labels), where
    for f in RESULT_FIELDS:
        assert getattr(ctx.result, f) == getattr(r.res, f), (where, f, getattr(ctx.result, f), getattr(r.res, f))


def assert_frames_equal_oracle(where, P, ctxs, labs, runs):
    for i, (ctx, lab, r) in enumerate(zip(ctxs, labs, runs)):
        w = "%s, frame %d (%s)" % (where, i, r.frame)
        if r.res.n_voxels:
            assert_equals_oracle(w, ctx, lab, r)
        else:
            assert_dead(w, P, ctx, lab, r)


def assert_context_state(where, P, ctx, r, params):
    """What a context answers after its batch, as test_vccs_getters_match_oracle asks a lone call: the supervoxel map, the adjacency and a recluster with another
    threshold, metric and merging mode against cluster() on the oracle's handle of the frame's lone run."""
    sv = ctx.supervoxels()
    cen = r.h.get("SV_CENTROID").reshape(-1, 10)
    assert np.array_equal(sv["label"], r.h.get("SV_LABELS")) and len(sv["label"]) == r.res.n_supervoxels, where
    for k, cols in (("xyz", slice(0, 3)), ("rgb", slice(3, 6)), ("normal", slice(6, 9))):
        assert first_mismatch(k, np.ascontiguousarray(cen[:, cols]), np.ascontiguousarray(sv[k]).reshape(-1, 3)) is None, (where, k)
    xyz, rgba, svlab = ctx.voxel_centroid_cloud()
    assert np.array_equal(svlab, r.h.get("VOXEL_SVLABEL")) and first_mismatch("VOXEL_XYZ", r.h.get("VOXEL_XYZ").reshape(-1, 3), xyz.reshape(-1, 3)) is None, where
    assert np.array_equal(ctx.supervoxel_adjacency().reshape(-1, 2), r.h.get("EDGES").reshape(-1, 2)), where
    want, n_merges, n_regions, _ = B.oracle_recluster(P, r, params)
    got = ctx.recluster(B.params_of(P, params, **B.RECLUSTER))
    assert np.array_equal(got, want) and (ctx.result.n_merges, ctx.result.n_regions) == (n_merges, n_regions), (where, int(ctx.result.n_merges), n_merges)


# ---- 1. one deep frame beside shallow ones ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [m.name for m in B.MIXES if m.kind == "depth"])
def test_a_deep_frame_sets_the_sort_widths_of_its_batch(P, oracle, monkeypatch, capfd, name):
    """Frames of depth 1, 2 and 3 sorted over the 3 D + 1 key bits of a frame of depth D = 13 .. 21: on the tile path while 3 D + tile_bits + 14 <= 64 (at depth 13 the
    deep frame alone takes the per-voxel table of d_vox_table / d_neighbors, its mates the block table, in one dispatch), refused for all before anything ran beyond,
    then with one-word keys while 3 D + 1 + idxbits <= 64 and as (key, index) pairs beyond -- reached here without F3DS_SORT_PAIRS.  Which of them (the test's name says
    it) follows from the oracle's depths, the point counts and the two formulas."""
    m = B.MIX[name]
    runs = B.runs_of(oracle, P, m)
    set_env(monkeypatch, dict(m.env, F3DS_TRACE_ERR="1"))
    monkeypatch.delenv("F3DS_SORT_PAIRS", raising=False)
    want = B.predict_stage0([int(r.res.octree_depth) for r in runs], [len(r.pts) for r in runs], len(runs), m.env["F3DS_VOX_TILES"])
    assert want == (m.expect["path"], m.expect["sort"])
    ctxs = contexts(P, len(runs))
    try:
        capfd.readouterr()
        labs = run_batch(P, ctxs, runs)
        err = capfd.readouterr().err
        assert [c.stage0_path() for c in ctxs] == [want[0]] * len(runs), name
        # a batch the tile path was open to and whose keys do not fit it starts over on the sort path before anything ran: the host says so, no frame is blamed and
        # no tile kernel has counted anything
        depths, n = [int(r.res.octree_depth) for r in runs], [len(r.pts) for r in runs]
        started_over = m.env["F3DS_VOX_TILES"] != "0" and len(runs) >= B.TILE_MIN_FRAMES and B.tile_key_bits(depths, n) > B.KEY_BITS
        assert REFUSED not in err and VOX_AGAIN.findall(err) == ([str(len(runs))] if started_over else []), err
        assert ("tile path: most voxels in a tile" in err) == (want[0] == "tiles"), err
        assert_frames_equal_oracle(name, P, ctxs, labs, runs)
        assert all(c.launch_shape()[2] == len(runs) for c in ctxs)
    finally:
        close_all(ctxs)


# ---- 2. one voxel beside 13 824 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [m.name for m in B.MIXES if m.kind == "size"])
def test_a_big_frame_sets_the_launch_widths_and_the_merge_layout_of_its_batch(P, oracle, monkeypatch, name):
    """Frames of 1, 4 and 1 025 voxels beside one of 13 824 whose 13 349 adjacencies fit no LDS layout with keys: every dispatch is as wide as the big frame needs, and
    all frames merge with global keys, (8, 0) -- alone the small ones take (8, 2).  As 16 frames: a sixteenth of the streaming width each, and d_normals_t<256>."""
    m = B.MIX[name]
    runs = B.runs_of(oracle, P, m)
    for k in ("F3DS_VOX_TILES", "F3DS_MERGE_NW", "F3DS_MERGE_KEYS", "F3DS_FORCE_GLOBAL_MERGE", "F3DS_NORMALS_THREADS", "F3DS_GRID_CAP", "F3DS_GRID_TARGET"):
        monkeypatch.delenv(k, raising=False)
    ctxs = contexts(P, len(runs))
    try:
        labs = run_batch(P, ctxs, runs)
        assert [c.merge_layout() for c in ctxs] == [m.expect["layout"]] * len(runs), name
        if "shape" in m.expect:
            assert [c.launch_shape() for c in ctxs] == [m.expect["shape"]] * len(runs), name
        else:
            assert all(c.launch_shape()[2] == m.expect["frames_in_shape"] for c in ctxs), name
        assert [c.stage0_path() for c in ctxs] == [B.predict_batch_path(runs, len(runs))] * len(runs) == [m.expect["path"]] * len(runs), name      # (the big frame's tiles hold 4096 voxels each: refused after the tile path ran)
        assert_frames_equal_oracle(name, P, ctxs, labs, runs)
        for i, (c, r) in enumerate(zip(ctxs, runs)):
            assert_context_state("%s, context %d (%s)" % (name, i, r.frame), P, c, r, m.params)
    finally:
        close_all(ctxs)
    if "lone_layout" in m.expect:
        for r in runs:
            if r.res.n_edges <= B.FIT_EDGES:
                ctx = fresh(P)
                try:
                    lab = ctx.segment(r.pts, r.prm)
                    assert ctx.merge_layout() == m.expect["lone_layout"] and ctx.launch_shape()[2] == 1, r.frame
                    assert_equals_oracle(r.frame + " alone", ctx, lab, r)
                finally:
                    ctx.close()


# ---- 3. frames that leave the batch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [m.name for m in B.MIXES if m.kind == "dead"])
def test_frames_without_voxels_leave_the_batch_and_the_rest_goes_on(P, oracle, monkeypatch, name):
    """An empty frame and an all-NaN frame as the first two of six (the call's owner, whose stream, argument arena and stage events the live frames go on using, is
    dead), another between live frames; a batch of dead frames only; a dead frame last.  Dead frames: every label F3DS_NO_LABEL and the oracle's counts; live frames:
    the oracle's arrays; and every context of the batch, dead or live, then segments a frame alone as a fresh one would."""
    m = B.MIX[name]
    runs = B.runs_of(oracle, P, m)
    monkeypatch.delenv("F3DS_VOX_TILES", raising=False)
    later = B.oracle_run(oracle, P, "block8", m.params)
    ctxs = contexts(P, len(runs))
    try:
        labs = run_batch(P, ctxs, runs)
        assert_frames_equal_oracle(name, P, ctxs, labs, runs)
        want_path = B.predict_batch_path(runs, len(runs))      # (the tile path goes by the contexts of the call, dead ones included: six, four of them dead, take it)
        assert all(c.stage0_path() == want_path for c, r in zip(ctxs, runs) if r.res.n_voxels), name
        for i, (c, r) in enumerate(zip(ctxs, runs)):
            lab = c.segment(later.pts, later.prm)
            assert_equals_oracle("%s, context %d (had %s) alone afterwards" % (name, i, r.frame), c, lab, later)
        labs = run_batch(P, ctxs, runs)      # ... and the same batch once more on the used contexts
        assert_frames_equal_oracle(name + ", second call", P, ctxs, labs, runs)
    finally:
        close_all(ctxs)


# ---- 4. what a context remembers of a refusal ------------------------------------------------------------------------------------------------------
def test_a_refused_context_keeps_its_batches_off_the_tile_path_for_its_penalty(P, oracle, monkeypatch, capfd):
    """The tile path refuses the frame of context 1 (a voxel of 257 points) after it ran: all four frames run again on the sort path.  The context then waits
    vox_dense_penalty = 8 calls that would have taken the tile path (calls 2 .. 9 go straight to the sort path, without a word), the tenth tries the tile path again,
    is refused again and doubles the penalty, the eleventh is silent again.  stage0_path() says "sort" for all four frames on every one of these calls.  The memory is
    the refused context's alone: its three mates and a fresh context take the tile path at once."""
    m = B.MIX["tile-refusal-memory"]
    runs = B.runs_of(oracle, P, m)
    dense = m.cond[1]
    set_env(monkeypatch, m.env)
    ctxs = contexts(P, len(runs))
    extra = None
    try:
        calls = B.DENSE_PENALTY + 3
        loud = (1, B.DENSE_PENALTY + 2)      # call 1, and the first call after `penalty` silent ones
        for call in range(1, calls + 1):
            capfd.readouterr()
            labs = run_batch(P, ctxs, runs)
            err = capfd.readouterr().err
            where = "call %d" % call
            if call in loud:
                assert err.count(REFUSED) == 1 and err.count(REFUSED_WHY) == 1 and VOX_AGAIN.findall(err) == [str(len(runs))], (where, err)
            else:
                assert REFUSED not in err and not VOX_AGAIN.findall(err) and "tile path:" not in err, (where, err)
            assert [c.stage0_path() for c in ctxs] == ["sort"] * len(runs), where
            if call in (1, 2, B.DENSE_PENALTY + 2):
                assert_frames_equal_oracle(where, P, ctxs, labs, runs)
            else:
                for lab, r in zip(labs, runs):
                    assert np.array_equal(lab, r.labels), (where, r.frame)
        extra = fresh(P)
        rest = [i for i in range(len(runs)) if i != dense]
        capfd.readouterr()
        labs = run_batch(P, [ctxs[i] for i in rest] + [extra], [runs[i] for i in rest] + [runs[0]])
        err = capfd.readouterr().err
        assert REFUSED not in err and not VOX_AGAIN.findall(err), err
        assert [c.stage0_path() for c in [ctxs[i] for i in rest] + [extra]] == ["tiles"] * 4
        assert_frames_equal_oracle("without the refused context", P, [ctxs[i] for i in rest] + [extra], labs, [runs[i] for i in rest] + [runs[0]])
    finally:
        close_all(ctxs + ([extra] if extra else []))


# ---- 5. one short adjacency list -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [m.name for m in B.MIXES if m.kind == "regrow"])
def test_one_short_adjacency_list_reruns_the_pass_of_every_frame(P, oracle, monkeypatch, capfd, name):
    """One context created under F3DS_EDGE_MULT = 1 with a frame of 18 792 adjacencies at S0 = 1 728 (room for 2 752, then 7 936, then 28 672), three contexts with the
    default room: the pass of all four runs again exactly twice, from cleared counters; the three frames that were rerun without needing it equal the oracle as the
    one that needed it does.  The room stays with the context: a second call prints nothing."""
    m = B.MIX[name]
    runs = B.runs_of(oracle, P, m)
    short = m.expect["short"]
    ctxs = []
    for i in range(len(runs)):      # (the switch is read when a context is created)
        set_env(monkeypatch, dict(F3DS_EDGE_MULT="1" if i == short else None))
        ctxs.append(fresh(P))
    set_env(monkeypatch, dict(m.env, F3DS_EDGE_MULT=None))
    try:
        for call, reruns in ((1, m.expect["reruns"]), (2, 0)):
            capfd.readouterr()
            labs = run_batch(P, ctxs, runs)
            err = capfd.readouterr().err
            assert ADJ_AGAIN.findall(err) == [str(len(runs))] * reruns, (name, call, err)
            assert_frames_equal_oracle("%s, call %d" % (name, call), P, ctxs, labs, runs)
        for i, (c, r) in enumerate(zip(ctxs, runs)):
            assert_context_state("%s, context %d (%s)" % (name, i, r.frame), P, c, r, m.params)
    finally:
        close_all(ctxs)


# ---- 6. incident-list pools that overflow in some frames ---------------------------------------------------------------------------------------------
def test_a_merge_stage_rerun_leaves_the_frames_that_had_finished_as_they_were(P, oracle, monkeypatch, capfd):
    """F3DS_ILIST_SLACK = 1: the frames of 215 and 960 merges overflow their incident-list pools, the frame without an adjacency (a pool of 16 entries that nothing
    enters) finishes at once -- and is merged again, from the untouched supervoxel state, when the stage of all four runs again (once where it was measured: four times
    the room was enough for both; nothing derives the count in advance).  All four equal the oracle, MERGES, SV_REGION and VOXEL_REGION included.  The
    multipliers stay with the contexts: with the switch removed a recluster with another threshold and metric equals cluster() on the oracle's handle, as do the getters."""
    m = B.MIX["merge-rerun-mix"]
    runs = B.runs_of(oracle, P, m)
    set_env(monkeypatch, m.env)
    monkeypatch.delenv("F3DS_VOX_TILES", raising=False)
    ctxs = contexts(P, len(runs))
    try:
        capfd.readouterr()
        labs = run_batch(P, ctxs, runs)
        err = capfd.readouterr().err
        again = MERGE_AGAIN.findall(err)
        print("merge-rerun-mix: the merge stage ran again %d times" % len(again))
        assert len(again) >= 1 and set(again) == {str(len(runs))} and MERGE_GLOBAL_AGAIN not in err, err
        assert_frames_equal_oracle(m.name, P, ctxs, labs, runs)
        monkeypatch.delenv("F3DS_ILIST_SLACK", raising=False)
        for i, (c, r) in enumerate(zip(ctxs, runs)):
            assert_context_state("%s, context %d (%s)" % (m.name, i, r.frame), P, c, r, m.params)
    finally:
        close_all(ctxs)
