"""The synthetic merge graphs of merge_graphs_common.py, checked without a GPU: the generator is deterministic, the oracle's run of every case meets the structural
condition the case is for (so no case can stop exercising its path unnoticed), the replay accepts every oracle log and refuses a damaged one, the oracle is invariant
under other keys and row orders, and the kernel constants the cases are sized by are the library's own (P.constant).

Oracle seconds per case on the development machine (each run is made once per process and shared): star400-to-the-end 1.1 - 1.3, star1099 0.6, grid30-all-equal 0.5,
chain-E8191 / E8192 / E8193 0.5 - 0.6 each, the three grids of 12 096 / 12 160 edges 0.7 - 0.8 each, the six tie17-lane chains (3 147 edges) 0.1 - 0.6 each (equalization the
most), chain-E4095 .. E4097 0.2 each, grid22-all-equal 0.2, star1024 .. star1026 and hubs 0.2 each, rest-and-resume 0.15, star1099-all-equal 0.1, everything else under 0.1:
about 10 s for the 109 cases, and 3 s more for the nine runs under other keys."""

import numpy as np
import pytest

import merge_graphs_common as G
from test_cluster_supervoxels import map_labels, relabel

NAMES = [c.name for c in G.CASES]


def test_generator_is_deterministic_and_well_formed():
    for kind, kw in (("star", dict(spokes=50)), ("tie_chain", dict(k=3, placement="lanes", normals="paired")), ("hubs", {}), ("rest", dict(pairs=3, chains=2, length=5)), ("grid", dict(w=5, h=4, pad=3))):
        a, pa = G.make_graph(kind, 3, **kw); b, pb = G.make_graph(kind, 3, **kw); c, pc = G.make_graph(kind, 4, **kw)
        assert np.array_equal(pa, pb) and all(np.array_equal(a[k], b[k]) for k in a)
        assert not all(np.array_equal(a[k], c[k]) for k in a)                          # the seed matters
        S = len(a["label"])
        assert a["voxel_offset"][0] == 0 and len(a["voxel_offset"]) == S + 1 and len(a["voxel_xyz"]) == a["voxel_offset"][-1] == len(a["voxel_rgba"])
        assert set(map(tuple, pa.tolist())) == set(map(tuple, pa[:, ::-1].tolist()))     # both directions
        assert np.array_equal(pa, pa[np.lexsort((pa[:, 1], pa[:, 0]))]) and len(set(map(tuple, pa.tolist()))) == len(pa)
        assert (a["voxel_rgba"] >> 24 == 0).all()


def test_every_supervoxel_of_every_case_is_a_plane_patch():
    """At least 4 voxels, coplanar and not collinear (a smaller region gets a degenerate normal after its first merge and merging stops) -- but for the single voxel the
    big-region chain absorbs on purpose."""
    for name in NAMES:
        sv, pairs = G.graph_of(name)
        cnt = np.diff(sv["voxel_offset"])
        assert (cnt >= 4).all() or (name == "big-single-leaves" and sorted(cnt.tolist())[:2] == [1, 4]), name
        first = sv["voxel_offset"][:-1][cnt >= 4].astype(np.int64); last = sv["voxel_offset"][1:][cnt >= 4].astype(np.int64) - 1
        p = sv["voxel_xyz"]
        u, v = p[first + 1] - p[first], p[last] - p[first]      # (the second voxel lies in the lattice's first row, the last one in another)
        assert (np.linalg.norm(np.cross(u, v), axis=1) > 0).all(), name


def test_kernel_constants_the_cases_are_sized_by(P):
    """MC_TL_CAP, MC_SP_TL, MC_SP_LEAVES, MC_GROUP, the staging chunks, the speculation's rest counter, the LDS limit, the initial event room and the reasons for a rerun
    of the stage: the library's own constants by name -- and the event room as the host computes it from them."""
    got = [(name, P.constant(name), want) for name, want in G.KERNEL_CONSTANTS.items()]
    assert len(got) == 18
    for name, have, want in got:
        assert have == want, "%s is %r, the tests assume %r" % (name, have, want)
    for E in (0, 1, 63, 4096, 12096, 1 << 20, 1 << 28):
        for mult in (G.EV_MULT, 4 * G.EV_MULT, 16384):
            assert P.policy_capacity(P.CAP_EVENTS, E, mult) == min(E * mult + G.EV_EXTRA, 0x7FFFFFFF), (E, mult)
    assert P.policy_grow(G.EV_MULT, P.constant("EV_MULT_CAP")) == 4 * G.EV_MULT


def test_largest_edge_count_whose_keys_fit_lds(P):
    lo, hi = 64, 1 << 16
    assert P.merge_layout_info(lo, 8, 2)[3] and not P.merge_layout_info(hi, 8, 2)[3]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if P.merge_layout_info(mid, 8, 2)[3] else (lo, mid)
    assert lo == G.FIT_EDGES
    total, sp_rows, ecap, fits = P.merge_layout_info(G.FIT_EDGES, 8, 2)
    assert fits and total <= G.MC_LDS_LIMIT and sp_rows == 128 < G.SP_ROWS8_MAX                   # the room for the second merge's rows has shrunk to its floor
    assert not P.merge_layout_info(G.FIT_EDGES + 64, 8, 2)[3] and P.merge_layout_info(G.FIT_EDGES + 64, 8, 0)[3]
    for e in (8191, 8192, 8193, 4095, 4096, 4097):                                               # the NGcap cases fit every layout they are run in
        assert all(P.merge_layout_info(e, nw, res)[3] for nw in (4, 8) for res in (0, 2))
    assert P.merge_layout_info(1099, 8, 2)[3] and P.merge_layout_info(1740, 4, 2)[3]             # the fallback cases fall back because of their lists, not their size


def test_the_case_list_is_the_one_the_issue_names():
    """Nothing is left out: families 1..9 are all there, every tie size in every placement at both ranks, every size edge."""
    fam = {c.family for c in G.CASES}
    assert fam == set(range(1, 10)) and len(G.CASES) == len(set(NAMES))
    for k in (2, 3, 17):
        for pl in ("group", "lane", "lanes"):
            for rank in ("min", "second"):
                for mode in ("manual", "adaptive", "equalization"):
                    assert "tie%d-%s-%s-%s" % (k, pl, rank, mode) in G.CASE
    for e in (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193):
        assert "chain-E%d" % e in G.CASE
    for f in (2, 3, 5, 7):
        assert {c.merging for c in G.CASES if c.family == f} == {G.MANUAL, G.ADAPTIVE, G.EQUALIZATION}
    assert {G.CASE[n].family for n in G.RELABELLED} == fam


@pytest.mark.parametrize("name", NAMES)
def test_oracle_run_meets_the_condition_the_case_is_for(oracle, P, name):
    r = G.oracle_run(oracle, P, name)                        # (replay() has validated the log: alive, adjacent regions; final partition = SV_REGION; region count)
    assert (P.MANUAL_LAMBDA, P.ADAPTIVE_LAMBDA, P.EQUALIZATION) == (G.MANUAL, G.ADAPTIVE, G.EQUALIZATION)
    G.check_condition(r, P)
    assert r.seconds < 4.0, "%s: %.1f s of oracle time" % (name, r.seconds)      # (about 2 s at the most where it was measured)
    kept = G.kept_edges(r.pairs)
    assert np.array_equal(r.edges, kept)                     # slot order of the kernels = order of the kept pairs


def test_replay_refuses_a_damaged_log(oracle, P):
    r = G.oracle_run(oracle, P, "ladder20-manual")
    G.replay(r.edges, r.merges, r.sv, r.sv_region, r.res.n_regions)
    bad = r.merges.copy(); bad[5, 1] = bad[0, 1]             # absorbs a region that is gone
    with pytest.raises(AssertionError):
        G.replay(r.edges, bad, r.sv, r.sv_region, r.res.n_regions)
    far = r.merges.copy(); far[0, :2] = (1, 39)              # joins two regions that do not touch
    with pytest.raises(AssertionError):
        G.replay(r.edges, far, r.sv, r.sv_region, r.res.n_regions)
    with pytest.raises(AssertionError):                      # one merge short: region count and partition differ
        G.replay(r.edges, r.merges[:-1], r.sv, r.sv_region, r.res.n_regions)
    with pytest.raises(AssertionError):
        G.replay(r.edges, r.merges[:-1], r.sv, None, r.res.n_regions)
    with pytest.raises(AssertionError):
        G.replay(r.edges, r.merges[:-1], r.sv, r.sv_region, None)


def test_replay_counts_on_a_graph_small_enough_to_do_by_hand():
    """Triangle 1-2-3 with a tail 3-4, merges (1,2) then (1,3) then (1,4)."""
    sv = dict(label=np.array([1, 2, 3, 4], np.uint32), voxel_offset=np.array([0, 4, 9, 15, 22], np.uint32))
    edges = np.array([[1, 2], [1, 3], [2, 3], [3, 4]], np.uint32)
    merges = np.array([[1, 2, 0], [1, 3, 0], [1, 4, 0]], np.uint32)
    rp = G.replay(edges, merges, sv, np.array([1, 1, 1, 1]), 1)
    assert rp.nt.tolist() == [3, 2, 1] and G.touched(rp).tolist() == [2, 1, 0]      # nt = deg(a) + deg(b) - 1
    assert rp.dups.tolist() == [1, 0, 0] and rp.reweighted.tolist() == [1, 1, 0]
    assert rp.rows_b.tolist() == [5, 6, 7] and rp.leaves_b.tolist() == [1, 1, 1] and rp.relation == ["shares", "shares", None]
    rp = G.replay(np.array([[1, 2], [3, 4], [5, 6], [2, 5]]), np.array([[1, 2, 0], [3, 4, 0], [5, 6, 0], [1, 5, 0]]), dict(label=np.arange(1, 7), voxel_offset=np.arange(7) * 4), None, 2)
    assert rp.relation == ["independent", "independent", "shares", None] and rp.leaves_b.tolist() == [1, 1, 1, 2] and rp.rows_b.tolist() == [4, 4, 4, 8]
    rp = G.replay(np.array([[1, 2], [3, 4], [2, 3]]), np.array([[1, 2, 0], [3, 4, 0]]), dict(label=np.arange(1, 5), voxel_offset=np.arange(5) * 4), np.array([1, 1, 3, 3]), 2)
    assert rp.relation == ["adjacent", None]


@pytest.mark.parametrize("name", G.RELABELLED)
def test_oracle_is_invariant_to_keys_and_row_order_on_every_family(oracle, P, name):
    r = G.oracle_run(oracle, P, name)
    sv2, pairs2, lut, perm, vox = relabel(r.sv, r.pairs, np.random.default_rng(21))
    rc, region, vlab, res2, h2 = oracle.cluster_supervoxels(sv2, pairs2, G.params_of(P, r.case))
    assert rc == 0 and (res2.n_merges, res2.n_regions, res2.n_edges) == (r.res.n_merges, r.res.n_regions, r.res.n_edges)
    m2 = h2.get("MERGES").reshape(-1, 3)
    assert np.array_equal(m2[:, 2], r.merges[:, 2]) and np.array_equal(m2[:, :2], map_labels(r.merges[:, :2], lut))
    want = r.sv_region[np.searchsorted(np.sort(r.sv["label"]), r.sv["label"][perm])]
    assert np.array_equal(region, map_labels(want, lut)) and np.array_equal(vlab, r.vlab[vox])
