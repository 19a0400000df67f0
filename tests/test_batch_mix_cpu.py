"""The batch mixes of batch_mix_common.py, checked without a GPU: the constants of the host logic the mixes are sized by are the ones in the sources, the oracle's lone
runs of every mix's frames meet the condition that makes the batch the mix it is named for (so no mix can stop exercising its decision unnoticed), and the emulation of
the device pipeline equals the oracle byte for byte on every frame under every parameter set a mix uses -- the frames of depth 16 to 21 and of one and four voxels among
them, which no golden case has -- and on the recluster the GPU test asks of the contexts afterwards.

Oracle seconds on the development machine: 4.4 s for block(24, 24, 24) with 1 330 merges, 1.0 s for the 64 x 64 plane, 0.2 s and less for every other frame."""
import numpy as np
import pytest

import batch_mix_common as B
import merge_graphs_common as G
import vccs_clouds_common as C
from merge_graphs_common import FIT_EDGES

RESULT_FIELDS = ("n_points", "n_finite", "n_voxels", "octree_depth", "n_seed_cells", "n_seeds", "n_supervoxels", "n_edges", "n_merges", "n_regions", "sweeps")


def test_host_constants_the_mixes_are_sized_by():
    """VT_CNT_BITS, F3DS_VT_TILE, N_BLOCK_DEPTH_MAX, the tile path's penalty of 8 calls and its doubling up to 1024, edge_mult = 32, the + 1024 and the * 4 of the
    adjacency list, the 16 frames of d_normals_t<256>, the 3072 and 2048 of the launch widths, the four contexts the tile path wants, the 16 entries of a short
    incident-list pool, and the two comparisons with 64 key bits together with the expressions they compare, read from their defining lines."""
    got = B.read_host_constants()
    assert len(got) == 21
    for name, pat, have, want in got:
        assert have == want, "%s: %s gives %r, the tests assume %r" % (name, pat, have, want)
    assert B.VT_TILE == C.VT_TILE


def test_the_two_formulas_at_their_boundaries():
    """3 maxd + tile_bits + 14 <= 64 and 3 maxd + 1 + idxbits <= 64, by hand: depth 16 is the deepest grid of the tile path, 17 with at most 4096 points the deepest of
    the one-word sort (64 bits exactly), and one more point than 4096 moves both."""
    assert [B.bits_for(x) for x in (0, 1, 2, 4095, 4096, 4618)] == [0, 1, 2, 12, 13, 13]
    assert B.tile_key_bits([1, 16], [1, 4096]) == 62 and B.tile_key_bits([17], [515]) == 65 and B.tile_key_bits([16, 2], [4097, 5]) == 63
    assert B.sort_key_bits([17, 3], [4096, 514]) == 64 and B.sort_key_bits([17], [4097]) == 65 and B.sort_key_bits([18], [515]) == 65
    assert B.predict_stage0([16], [515], 4, None) == ("tiles", None) and B.predict_stage0([16], [515], 3, None) == ("sort", "one-word")
    assert B.predict_stage0([16], [515], 4, "0") == ("sort", "one-word") and B.predict_stage0([21], [515], 4, None) == ("sort", "pairs")


def test_the_mix_list_is_the_one_the_issue_names():
    kinds = {m.kind for m in B.MIXES}
    assert kinds == {"depth", "size", "dead", "refusal", "regrow", "rerun"} and len(B.MIXES) == 21
    depth = [m for m in B.MIXES if m.kind == "depth"]
    assert len(depth) == 12 and {m.frames[3] for m in depth} == {"far13", "far16", "far17", "far18", "far21", "far17-wide"}
    assert all(m.frames[:3] == ("one-point", "block3x1x1", "block8") for m in depth)
    assert all((m.expect["path"] + ("-" + m.expect["sort"] if m.expect["sort"] else "")) in m.name for m in depth)      # the predicted sort form is part of the test id
    assert {m.env["F3DS_VOX_TILES"] for m in depth} == {None, "0"}
    assert len(B.MIX["size-mix-16"].frames) == 16 == B.NORMALS_256_FRAMES and B.MIX["size-mix-16"].expect["shape"] == (192, 2048, 16)
    assert [m.frames for m in B.MIXES if m.kind == "dead"] == [("empty", "all-nan", "block8", "one-point", "all-nan", "block3x1x1"), ("empty", "all-nan", "empty", "all-nan"), ("block8", "empty")]
    assert B.MIX["tile-refusal-memory"].frames.index("one-dense-257") != 0
    assert B.STATE_MIXES == ["size-mix", "size-mix-16", "adjacency-regrow-mix-short-first", "adjacency-regrow-mix-short-last", "merge-rerun-mix"]
    assert FIT_EDGES == 12096


@pytest.mark.parametrize("name", B.NAMES)
def test_oracle_runs_meet_the_condition_of_the_mix(oracle, P, name):
    m = B.MIX[name]
    runs = B.runs_of(oracle, P, m)
    print(name, [(r.frame, "depth %d, V %d, S0 %d, S %d, E %d, merges %d, %.2f s" % (r.res.octree_depth, r.res.n_voxels, r.res.n_seeds, r.res.n_supervoxels, r.res.n_edges, r.res.n_merges, r.seconds)) for r in runs])
    B.check_condition(m, runs)
    assert all(r.seconds < (8.0 if r.frame == "block24-random" else 2.0) for r in runs), [(r.frame, r.seconds) for r in runs]


def test_no_mix_reaches_the_merge_rerun_with_the_global_memory_kernel(oracle, P):
    """What the mixes leave out: a merge whose two regions touch more than MC_TL_CAP = 1024 adjacencies sends the whole batch to d_merge.  The oracle's
    merge logs of the frames with the most merges, replayed on region adjacency sets, stay far below: in the 24 x 24 x 24 block the two regions of one merge have 265
    adjacencies between them (deg a + deg b; the touched list leaves the merged one out at either end: 263 entries), every other frame fewer."""
    most = {}
    for frame in ("block24-random", "block14-random", "plane64-grey", "count4097"):
        r = B.oracle_run(oracle, P, frame, "manual-2r")
        labels = r.h.get("SV_LABELS")
        rp = G.replay(r.h.get("EDGES").reshape(-1, 2), r.h.get("MERGES").reshape(-1, 3), dict(label=labels, voxel_offset=np.arange(len(labels) + 1)), None, r.res.n_regions)
        most[frame] = int(G.touched(rp).max())
    print(most)
    assert max(most.values()) == most["block24-random"] == 265 - 2 and 2 * 265 < G.MC_TL_CAP, most


@pytest.mark.parametrize("frame,params", B.PAIRS, ids=["%s-%s" % p for p in B.PAIRS])
def test_emulation_equals_the_oracle_on_every_frame(oracle, emul, P, frame, params):
    """Labels, the counts of the Result and every debug array; the frames of the table have the depth the table says."""
    r = B.oracle_run(oracle, P, frame, params)
    er = C.emul_run(emul, r.pts, r.prm)
    assert er.rc == 0
    if frame in B.DEPTH_OF:
        assert r.res.octree_depth == B.DEPTH_OF[frame]
    assert C.emul_equals_oracle(er, r.labels, r.h) is None
    for f in RESULT_FIELDS:
        assert getattr(er.res, f) == getattr(r.res, f), f
    if r.res.n_voxels and any(frame in B.MIX[n].frames and B.MIX[n].params == params for n in B.STATE_MIXES):
        # the recluster the contexts are asked for after their batch: the emulation's cluster() on its own handle against the oracle's
        want, n_merges, n_regions, _ = B.oracle_recluster(P, r, params)
        rc, got, res = er.h.cluster(B.params_of(P, params, **B.RECLUSTER), len(r.pts))
        assert rc == 0 and np.array_equal(got, want) and (res.n_merges, res.n_regions) == (n_merges, n_regions)
        print("%s, %s: %d merges and %d regions, reclustered %d and %d" % (frame, params, r.res.n_merges, r.res.n_regions, n_merges, n_regions))
        if frame.endswith("-random") and params == "manual-2r":      # (on random colours the other parameters give another clustering: the recluster is no repetition; supervoxels of one voxel never merge)
            assert (n_merges, n_regions) != (int(r.res.n_merges), int(r.res.n_regions)), (n_merges, n_regions)
