"""The seed-stage clouds of seed_clouds_common.py, checked without a GPU: the brute-force reference gives what a hand count gives, the census of every case (taken from the
reference alone) meets the condition the case is for, reference = oracle = emulation on SEED_ORIG, SEED_KEPT and n_seed_cells -- which is the check that the oracle's
restriction to 27 cells is sound on these clouds --, the emulation equals the oracle on every debug array, and the constants and margins of the seed kernels the cases are
sized by are the library's own (P.constant)."""

import numpy as np
import pytest

import seed_clouds_common as S
from conftest import ALL_DEBUG, first_mismatch

_emul = {}


def emul_run(emul, P, name):
    if name not in _emul:
        _emul[name] = emul.segment(S.frame_of(name), S.params_of(P, name))
    return _emul[name]


def test_reference_gives_what_a_hand_count_gives():
    """Two cells at seed_res = 4 voxels, the grid starting at voxel 0: voxel 0 at the origin, voxels at 1, 2.5 and 6 on x.  Cells [0, 4) and [4, 8) on x, centres at 2 and 6 (and 2 off the line on y and z):
    voxel 2 (at 2.5) is nearest to the first, voxel 3 to the second; voxel 4 at 12 makes the cube grow once.  Radius 2: voxel 2 counts itself and voxel 1."""
    u = 1.0 / 64
    xyz = np.array([(0, 0, 0), (1, 0, 0), (2.5, 0, 0), (6, 0, 0), (12, 0, 0)], np.float32) * np.float32(u)
    ref = S.reference(xyz, 4 * u, u)
    assert [e.trigger for e in ref.grid.events] == [0, 3, 4] and ref.grid.depth == 3 and [e.upper for e in ref.grid.events[1:]] == [(True, False, False)] * 2
    assert ref.grid.keys[:, 0].tolist() == [1, 1, 1, 2, 4] and len(set(ref.grid.keys[:, 1].tolist())) == 1
    assert np.allclose(ref.grid.min, (-4 * u, -28 * u, -28 * u))
    assert ref.seed_orig.tolist() == [2, 3, 4] and ref.num.tolist() == [2, 1, 1]
    assert ref.r2 == np.float32(4 * u * u) and abs(float(ref.min_points) - 0.05 * 4 * np.pi) < 1e-6
    assert ref.keep.tolist() == [True, True, True]
    cen = S.census(xyz, 4 * u, u, ref)
    assert [c.n_own for c in cen.cells] == [3, 1, 1] and [c.n_block for c in cen.cells] == [4, 4, 1] and cen.chunk_pos == [0, 3, 4]
    assert [float(c.own_min) for c in cen.cells] == [8.25 * u * u, 8 * u * u, 12 * u * u] and not any(c.shortcut for c in cen.cells) and not any(c.other_cell or c.tied for c in cen.cells)
    assert S.morton(np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0]]), 2).tolist() == [4, 2, 1, 32]


def test_seed_kernel_constants_the_cases_are_sized_by(P):
    """SEED_CHUNK = 256 and the 256 chunk boxes of a trip of d_seed_grow (its BLOCK), the stride 256 of the three candidate loops, four cells per workgroup (a wave each
    of the kernels' 256 threads; their launches divide by the same constant), F3DS_MAX_SEED_EVENTS, the margins 1e-3 and 1.001 and the 2^-23 of its largest coordinate
    the half cell gives up -- the library's own constants by name, the margins bit for bit as doubles --, and the two strict comparisons of the filter by the cases that
    sit on them from both sides."""
    got = [(name, P.constant(name), want) for name, want in S.SEED_CONSTANTS.items()]
    assert len(got) == 10
    for name, have, want in got:
        assert have == want and type(have) is type(want), "%s is %r, the tests assume %r" % (name, have, want)
    assert len(S.FILTER_BOUNDARY_CASES) == 2 and set(S.FILTER_BOUNDARY_CASES.values()) <= set(S.NAMES)
    assert S.CASE["c9-min-points-exactly-2"].cond == ("exact_min_points", 2) and S.CASE["c2-at-the-radius"].cond == ("at_r2",)


def test_the_case_list():
    assert S.NAMES == [
        "a1-single-cell", "a2-triggers-at-0-255-256", "a3-two-events-in-a-chunk", "a4-event-at-the-last-voxel", "a5-every-direction", "a6-thirteen-events", "a7-cube-edge",
        "a8-second-chunk-trip", "a9-thirteen-events-desc", "b1-shortcut-and-not", "b2-b7-corner-cut", "b3-ties", "b4-key-zero", "b5-cell-sizes", "b6-big-blocks", "c1-counts",
        "c2-at-the-radius", "c3-eight-cells", "c4-own-cell-only", "c5-pruned-neighbours", "c6-every-seed-dropped", "c7-every-seed-kept", "c8-face-near-the-radius",
        "c9-min-points-exactly-2", "d-offset-600", "d-offset-0"]
    assert set(S.BATCH) <= set(S.NAMES) and len(S.BATCH) == 4 and len({tuple(sorted(S.CASE[n].params.items())) for n in S.BATCH}) == 1
    assert set(S.NARROW) <= set(S.NAMES)
    assert S.min_points(S.EXACT_SEED_RES, S.RD) == np.float32(2.0)
    d = S.CASE["d-offset-600"].params
    assert (d["seed_res"], d["voxel_res"], d["use_transform"]) == (0.08, 0.008, 0) and (S.D_PAIRS, S.D_SEED) == (600, 1)


@pytest.mark.parametrize("name", S.NAMES)
def test_condition_holds_and_reference_oracle_and_emulation_agree(oracle, emul, P, name):
    r = S.oracle_run(oracle, P, name)
    cen, ref = r.census, r.census.ref
    print("%s: V %d, cells %d, kept %d, events %s, shortcut %d, other cell %d (under the bound %d), tied %d, most in a cell %d / in 27 cells %d, oracle %.2f s" % (
        name, cen.V, cen.C, int(ref.keep.sum()), [(e.trigger, e.depth) for e in cen.events], sum(c.shortcut for c in cen.cells), sum(c.other_cell for c in cen.cells),
        sum(c.shortcut and c.other_cell for c in cen.cells), sum(c.tied for c in cen.cells), max(c.n_own for c in cen.cells), max(c.n_block for c in cen.cells), r.seconds))
    S.check_condition(r)
    # the brute force over all voxels against the oracle's 27 cells
    assert r.res.n_seed_cells == cen.C and r.res.octree_depth >= 0
    assert S.equals("SEED_ORIG (reference, oracle)", ref.seed_orig, r.h.get("SEED_ORIG")) is None
    assert S.equals("SEED_KEPT (reference, oracle)", ref.seed_kept, r.h.get("SEED_KEPT")) is None
    assert r.res.n_seeds == len(ref.seed_kept)
    # the emulation of the device pipeline
    rc, elab, eres, eh = emul_run(emul, P, name)
    assert rc == 0 and eres.n_seed_cells == cen.C
    assert S.equals("SEED_ORIG (reference, emulation)", ref.seed_orig, eh.get("SEED_ORIG")) is None
    assert S.equals("SEED_KEPT (reference, emulation)", ref.seed_kept, eh.get("SEED_KEPT")) is None
    problems = [m for m in (first_mismatch(w, r.h.get(w), eh.get(w)) for w in ALL_DEBUG) if m]
    assert not problems, "\n".join(problems)
    assert np.array_equal(elab, r.labels)
    assert r.seconds < (6.0 if name.startswith("a8") else 1.0), "%s: %.1f s of oracle time" % (name, r.seconds)


def test_large_offset_census():
    """Family D on the reference alone, without the oracle (one point per voxel: the voxel centroids are the points, in the order the frame has them -- the order decides
    ordinals only, and no distance is tied here): at 600 m at least three cells whose own voxel is under the old shortcut bound while another cell's voxel is strictly
    nearer in float32; at 0 m none."""
    for name, want in (("d-offset-600", True), ("d-offset-0", False)):
        prm = S.CASE[name].params
        cen = S.census(S.frame_of(name)[:, :3], prm["seed_res"], prm["voxel_res"])
        bad = [c for c in cen.cells if c.shortcut and c.other_cell]
        print(name, len(bad), "of", cen.C)
        assert not any(c.tied for c in cen.cells)
        assert (len(bad) >= 3) if want else not bad
