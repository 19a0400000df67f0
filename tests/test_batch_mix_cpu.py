"""The batch mixes of batch_mix_common.py, checked without a GPU: the constants of the host logic the mixes are sized by are the library's own (P.constant; its batch-wide formulas compute what the restatement here computes), the oracle's lone
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


def test_host_constants_the_mixes_are_sized_by(P):
    """VT_CNT_BITS, VT_TILE, N_BLOCK_DEPTH_MAX, the tile path's penalty of 8 calls and its doubling up to 1024, edge_mult = 32, the + 1024 and the * 4 of the
    adjacency list, the caps of the four multipliers, the 16 frames of d_normals_t<256>, the 3072, 8 and 2048 of the launch widths, the four contexts the tile path
    wants, the extra entries of the incident-list pool, the 64 key bits and the three reasons for a rerun the mixes read in the trace: the library's own constants."""
    got = [(name, P.constant(name), want) for name, want in B.HOST_CONSTANTS.items()]
    assert len(got) == 25
    for name, have, want in got:
        assert have == want, "%s is %r, the tests assume %r" % (name, have, want)
    assert B.VT_TILE == C.VT_TILE
    with pytest.raises(P.F3dsError):
        P.constant("NO_SUCH_LIMIT")
    assert set(B.HOST_CONSTANTS) <= set(P.constants())


def test_the_stage0_plan_is_the_restated_one(P):
    """What segment_batch decides for stage 0 (P.stage0_plan: the function it calls) against predict_stage0, tile_key_bits and sort_key_bits: the path, the tile bits
    (maxtiles - 1), the index bits (maxn - 1, or pairs past 64 key bits), the sort width (3 maxd + 1), at every depth, at the point counts either side of a tile and of
    an index bit, at calls either side of four contexts and under every value of the two switches."""
    cases = 0
    for d in B.PLAN_DEPTHS:
        for n in B.PLAN_POINTS:
            for nctx in B.PLAN_CONTEXTS:
                for vt in B.PLAN_VOX_TILES:
                    for pairs in (False, True):
                        tiles, tile_bits, idxbits, sort_bits = P.stage0_plan(d, n, nctx, 1 if vt is None else int(vt), int(pairs))
                        path, form = B.predict_stage0([d], [n], nctx, vt, pairs)
                        what = (d, n, nctx, vt, pairs)
                        assert tiles == (path == "tiles"), what
                        assert tile_bits == B.tile_key_bits([d], [n]) - 3 * d - B.VT_CNT_BITS, what
                        assert sort_bits == 3 * d + 1, what
                        assert idxbits == (-1 if pairs or B.sort_key_bits([d], [n]) > B.KEY_BITS else B.sort_key_bits([d], [n]) - sort_bits), what
                        assert form is None or (form == "pairs") == (idxbits < 0), what
                        cases += 1
    assert cases == 21 * 8 * 4 * 3 * 2
    assert P.stage0_plan(16, 515, 4)[0] and not P.stage0_plan(16, 515, 3)[0] and P.stage0_plan(16, 515, 3, 2)[0] and not P.stage0_plan(17, 515, 4)[0]


def test_the_capacities_and_their_growth_are_the_restated_ones(P):
    """The adjacency list's room S0 * mult + 1024 and its growth as adjacency_room / regrows_needed restate them, the four multipliers' growth up to their caps, the
    penalty of a refusal, and the launch shape of a call: 256 threads per normals tile from 16 frames on, 3072 workgroups shared among the frames but 8 at the least
    and 2048 at the most, 2048 for a gathering kernel, F3DS_GRID_CAP in place of both."""
    for S0 in (0, 1, 9, 1728, 12289, 1 << 20, (1 << 30) - 2):
        for mult in (1, 4, 16, 32, 128, 1 << 14):
            assert P.policy_capacity(P.CAP_EDGES, S0, mult) == B.adjacency_room(S0, mult), (S0, mult)
    for E, S0 in ((18792, 1728), (1, 1), (100000, 9)):
        mult, k = 1, 0
        while E > P.policy_capacity(P.CAP_EDGES, S0, mult):
            mult = P.policy_grow(mult, P.constant("EDGE_MULT_CAP")); k += 1
        assert k == B.regrows_needed(E, S0, 1), (E, S0)
    for cap in (1 << 14, 16384, 64, 4096):
        m, seen = 1, []
        while P.policy_grow(m, cap) != m:
            m = P.policy_grow(m, cap); seen.append(m)
        assert seen == [B.EDGE_GROW ** (i + 1) for i in range(len(seen))] and m == cap
    assert P.policy_grow(32, 1 << 14) == 128 and P.policy_grow(8192, 1 << 14) == 32768      # (from EDGE_MULT = 32 the last step passes the cap: below it, one more step)
    p, seen = B.DENSE_PENALTY, []
    for _ in range(9):
        p = P.policy_dense_penalty(p); seen.append(p)
    assert seen == [16, 32, 64, 128, 256, 512, 1024, 1024, 1024] and seen[-1] == B.DENSE_PENALTY_CAP
    for frames in (1, 2, 3, 4, 15, 16, 17, 192, 384, 385, 1000):
        want_cap = min(max(B.GRID_TARGET // frames, 8), B.WIDE_CAP)
        assert P.policy_launch(frames) == (256 if frames >= B.NORMALS_256_FRAMES else 384, want_cap, B.WIDE_CAP), frames
        assert P.policy_launch(frames, normals_forced=256)[0] == 256 and P.policy_launch(frames, normals_forced=384)[0] == 384
        assert P.policy_launch(frames, grid_cap_forced=5)[1:] == (5, 5) and P.policy_launch(frames, grid_target=0)[1] == B.WIDE_CAP
    assert P.policy_launch(16)[1:] == B.MIX["size-mix-16"].expect["shape"][:2]
    # the incident-list pool of a frame without adjacencies: 16 entries under a short slack, 1024 otherwise; with adjacencies 2 E + slack * E * mult + extra, bounded by what the merges can need
    assert P.policy_capacity(P.CAP_ILIST, 0, 1, n_seeds=1, slack=1) == B.ILIST_SHORT_EXTRA and P.policy_capacity(P.CAP_ILIST, 0, 1, n_seeds=1, slack=32) == 1024
    assert P.policy_capacity(P.CAP_ILIST, 100, 4, n_seeds=1000, slack=3) == 200 + 3 * 100 * 4 + B.ILIST_SHORT_EXTRA
    assert P.policy_capacity(P.CAP_ILIST, 100, 4, n_seeds=2, slack=32) == 200 + 1 * (1024 + 512 + 4) + 1024


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
