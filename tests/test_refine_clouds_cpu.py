"""refineSupervoxels on the lattice clouds, checked without a GPU: the case list of refine_clouds_common.py meets the conditions that make it reach d_reseed's tie rule (per
thread and across threads), reseed collisions with and without sweeps behind them, erased helpers, ghost leaves of the seed stage that are alive when refine starts, the
wrap of the memo tag inside a refine iteration and the tiles that overflowed d_normals_t's tables; the numpy census those conditions are read from predicts the seeds the
oracle's run shows; the emulation's refine -- which scans and reduces as d_reseed's 256 threads do -- equals the oracle's on every case and iteration count, all seven arrays;
and the census table in refine_clouds_common's docstring is what the census gives.

Seconds on the development machine: 11 s for the 92 tests, 8 of them the three every-voxel cases (a reseed of theirs is 150 M distances, in the oracle, in the emulation
and in the census).

The tie rule, mutated in a scratch copy of the emulation: with `od < md` alone in the reduction (no `ob < mb`) the comparison below fails on r-tiny-supervoxels-desc,
d-deep-chain-cold, n-line-V127, s-voxel-of-256-points, g-seed-ghosts-one-sweep and g-seed-ghosts-two-sweeps at every k, on d-deep-chain-desc at k = 1, 2 and on t-plane24 at
k = 2, 3 -- the cases and iterations whose census counts reduction_ties, r-helpers-of-64-and-65-leaves excepted (its ties lie inside isolated 2 x 2 crumbs that regrow
alike from any of their four voxels).  With `d <= bd` in a thread's scan (the last minimum stays) it fails on r-holes-same-thread-tie at every k and passes everywhere
else: no other case has two tied voxels in one thread."""

import numpy as np
import pytest

import refine_clouds_common as RC
import vccs_clouds_common as C

PAIRS = [(c.name, k) for c in RC.CASES for k in c.ks]


def test_reseed_block_is_the_one_in_the_source(P):
    """d_reseed::BLOCK: the census sorts ties by ordinal % 256.  The kernel sizes its two LDS arrays by BLOCK and starts its reduction at BLOCK / 2, so the one number
    is all there is to restate; that the reduction halves down to one thread needs a power of two, and what the scan stride and the reduction's tie clause decide is
    held by the cases whose census counts two tied voxels in one thread (256 apart) and ties the reduction decides."""
    facts = [P.constant("d_reseed::BLOCK") == RC.RESEED_BLOCK, RC.RESEED_BLOCK & (RC.RESEED_BLOCK - 1) == 0,
             "r-holes-same-thread-tie" in RC.CASE, "n-line-V127" in RC.CASE and "r-tiny-supervoxels-desc" in RC.CASE]
    assert len(facts) == 4 and all(facts), facts


def test_the_case_list_is_the_one_the_issue_names():
    for n in ("r-tiny-supervoxels-desc", "r-helpers-of-64-and-65-leaves", "d-deep-chain-cold", "d-deep-chain-desc", "r-every-voxel-a-seed-12287", "r-every-voxel-a-seed-12288",
              "r-every-voxel-a-seed-12289", "w-corridor-ratio40", "w-corridor-ratio72", "n-ring1-456-over", "n-ring2-901-over", "r-tile-lists-of-15-and-17", "t-plane24", "v-transform"):
        assert n in RC.CASE and RC.CASE[n].build is None and n in C.CASE
    assert len(RC.CASES) == len(RC.CASE) == 21
    assert all(max(RC.CASE[n].ks) <= 2 for n in RC.EVERY_VOXEL) and any(RC.CASE[n].ks == (1, 2) for n in RC.EVERY_VOXEL)
    assert all(c.ks == (1, 2, 3) for c in RC.CASES if c.name not in RC.EVERY_VOXEL)
    assert all(n in RC.CASE for n in RC.GHOST_CASES + RC.WRAP_CASES + RC.OVERFLOW_CASES)


def test_census_counts_what_a_hand_count_gives():
    """600 voxels on a line, one unit apart.  A centroid half way between voxels 10 and 11 ties them in one thread's neighbourhood (10 % 256 < 11 % 256: the scan order of
    the threads decides nothing the reduction's first clause would not); one at voxel 300's place has no tie; one half way between 255 and 256 ties across threads the
    other way round (256 % 256 = 0 < 255: only `ob < mb` keeps the lower ordinal); two centroids near voxel 40 collide; helper 4 of 7 is not live; one half way between
    voxels 1 and 2 ties them in ascending threads, and yet the reduction alone would end on 2: its last step lets the even threads' best stand against the odd ones'."""
    xyz = np.zeros((600, 3), np.float32); xyz[:, 0] = np.arange(600)
    cen = np.zeros((6, 3), np.float32); cen[:, 0] = (10.5, 300.0, 255.5, 40.25, 39.75, 1.5)
    c = RC.reseed_census_of(xyz, 7, [1, 2, 3, 5, 6, 7], cen)
    assert (c.live, c.ties, c.cross_thread_ties, c.reduction_ties, c.same_thread_ties, c.collisions, c.erased) == (6, 3, 1, 2, 0, 1, 1)
    assert c.seeds.tolist() == [10, 300, 255, -1, 40, 40, 1]
    assert [RC.reduction_winner_without_tie_clause(np.array(w)) for w in ([10, 11], [255, 256], [1, 2], [5, 261], [3, 261, 517], [128, 129, 384])] == [10, 256, 2, 5, 261, 128]
    assert RC.reseed_census_of(np.concatenate([xyz, xyz[5:6]]), 1, [1], np.array([[5.0, 0, 0]], np.float32))[1:5] == (1, 0, 1, 0)      # voxels 5 and 600 at one place: threads 5 and 88, and the reduction prefers 88
    far = np.concatenate([xyz[:517], xyz[5:6]])                                                                                      # voxels 5 and 517 (= 5 + 2 * 256): one thread scans both
    assert RC.reseed_census_of(far, 1, [1], np.array([[5.0, 0, 0]], np.float32))[1:5] == (1, 0, 0, 1)
    d = RC.sqdist32(np.array([[0.1, 0.2, 0.3]], np.float32), np.array([[1.7, -2.9, 0.05]], np.float32))
    a, b, e = (np.float32(0.1) - np.float32(1.7)), (np.float32(0.2) - np.float32(-2.9)), (np.float32(0.3) - np.float32(0.05))
    assert d.dtype == np.float32 and d[0, 0] == np.float32(np.float32(np.float32(a * a) + np.float32(b * b)) + np.float32(e * e))


# ---- the conditions the case list has to meet (conditions, not measurements: a case that stops meeting its condition stops testing what it is in the list for)
def test_condition_1_a_reseed_with_at_least_100_ties(oracle, P):
    assert RC.reseed_census(oracle, P, "r-tiny-supervoxels-desc", 1).ties >= 100


def test_condition_2_ties_the_reduction_decides(oracle, P):
    r = RC.oracle_run(oracle, P, "r-tiny-supervoxels-desc")
    assert r.census.V > RC.RESEED_BLOCK
    for k in (1, 2):
        c = RC.reseed_census(oracle, P, "r-tiny-supervoxels-desc", k)
        assert c.cross_thread_ties >= 1 and c.reduction_ties >= 1, (k, c[:5])
    # ... also where fewer voxels than threads leave most of the reduction's inputs empty, and behind a collision
    for name in ("n-line-V127", "s-voxel-of-256-points", "d-deep-chain-cold", "g-seed-ghosts-one-sweep", "g-seed-ghosts-two-sweeps"):
        assert RC.reseed_census(oracle, P, name, 1).reduction_ties >= 1, name
    # the ascending scan of ONE thread decides a seed where two tied voxels are a multiple of 256 ordinals apart
    assert RC.reseed_census(oracle, P, "r-holes-same-thread-tie", 1).same_thread_ties >= 1 and RC.oracle_run(oracle, P, "r-holes-same-thread-tie").census.V > 2 * RC.RESEED_BLOCK


def test_condition_3_a_reseed_collision_with_sweeps_behind_it(oracle, P):
    for name, k in (("d-deep-chain-cold", 1), ("g-seed-ghosts-two-sweeps", 1), ("g-seed-ghosts-two-sweeps", 2), ("g-seed-ghosts-two-sweeps", 3)):
        assert RC.reseed_census(oracle, P, name, k).collisions >= 1 and RC.oracle_run(oracle, P, name).census.sweeps >= 1, (name, k)


@pytest.mark.parametrize("name", RC.EVERY_VOXEL)
def test_condition_4_mass_collision_without_a_sweep(oracle, P, name):
    r = RC.oracle_run(oracle, P, name)
    for k in RC.CASE[name].ks:
        c = RC.reseed_census(oracle, P, name, k)
        assert r.census.sweeps == 0 and c.erased == 0 and c.collisions == r.census.S0 - 1 and c.live == r.census.S0, (name, k, c[:7])
        assert len(RC.oracle_refine(oracle, P, name, k)["label"]) == r.census.S0           # ghost-only helpers stay supervoxels


def test_condition_5_a_quarter_of_the_helpers_erased(oracle, P):
    for name in ("r-tiny-supervoxels-desc", "d-deep-chain-cold"):
        S0 = RC.oracle_run(oracle, P, name).census.S0
        assert any(4 * RC.reseed_census(oracle, P, name, k).erased >= S0 for k in (2, 3)), name
    # ... and the helpers the refine itself erased: more on entry to iteration 2 than on entry to iteration 1
    assert RC.reseed_census(oracle, P, "r-tiny-supervoxels-desc", 2).erased >= RC.reseed_census(oracle, P, "r-tiny-supervoxels-desc", 1).erased + 100


def test_condition_6_seed_stage_ghosts_alive_when_refine_starts(emul, P):
    """... and, in one case at least, with a higher label than the owner of the voxel they hold: there `every helper that holds it` (the oracle) and `ghost_active` (the
    device) decide whose refineNormals writes the voxel last, and the comparison of voxel_normal below proves them the same."""
    for name in RC.GHOST_CASES:
        assert RC.ghosts_alive_on_entry(emul, P, name, 1) >= 1, name
    assert RC.ghosts_above_owner_on_entry(emul, P, "g-seed-ghosts-one-sweep", 1) >= 1 and RC.ghosts_above_owner_on_entry(emul, P, "d-deep-chain-cold", 1) >= 1
    assert RC.ghosts_alive_on_entry(emul, P, "g-seed-ghosts-two-sweeps", 3) >= 1            # reseed-made ghosts that two sweeps leave alive
    assert all(RC.ghosts_alive_on_entry(emul, P, n, 1) == 0 for n in RC.NAMES if n not in RC.GHOST_CASES)


def test_condition_7_a_refine_iteration_past_the_memo_tag_wrap(oracle, P):
    assert [RC.oracle_run(oracle, P, n).census.sweeps for n in RC.WRAP_CASES] == [71, 128] and C.TAG_PERIOD == 63
    assert all(2 in RC.CASE[n].ks for n in RC.WRAP_CASES)


def test_condition_8_tiles_that_overflowed_the_normals_tables(oracle, P):
    for n in RC.OVERFLOW_CASES:
        assert RC.oracle_run(oracle, P, n).census.overflow.any() and RC.oracle_run(oracle, P, n).census.fits.any(), n


def test_cases_with_fewer_voxels_than_reseed_threads(oracle, P):
    """Threads of d_reseed that see no voxel enter the reduction with best = -1, bd = 0."""
    assert sorted(RC.oracle_run(oracle, P, n).census.V for n in ("s-chunk-straddle", "n-line-V127", "s-voxel-of-256-points")) == [65, 127, 145]


# ---- the census against the oracle's own run, the emulation against the oracle
@pytest.mark.parametrize("name", ["g-seed-ghosts-no-sweep", "r-every-voxel-a-seed-12287"])
def test_census_predicts_the_seeds_of_a_run_without_sweeps(oracle, P, name):
    """Without a sweep the refined labels ARE the seeds: a voxel's label is the highest helper the census seeds there (addLeaf overwrites the owner in list order),
    every other voxel has none.  A census that rounded otherwise than a_sqdist, or broke ties otherwise than by the lowest ordinal, would name other voxels."""
    r = RC.oracle_run(oracle, P, name)
    assert r.census.sweeps == 0
    for k in RC.CASE[name].ks:
        c = RC.reseed_census(oracle, P, name, k)
        want = np.zeros(r.census.V, np.uint32)
        live = np.nonzero(c.seeds >= 0)[0]
        np.maximum.at(want, c.seeds[live], (live + 1).astype(np.uint32))
        got = RC.oracle_refine(oracle, P, name, k)
        assert np.array_equal(got["voxel_label"], want), (name, k, int((got["voxel_label"] != want).sum()))
        assert np.array_equal(got["label"], (live + 1).astype(np.uint32)) and (got["n_voxels"] == 1).all()


@pytest.mark.parametrize("name,k", PAIRS)
def test_emulation_refine_equals_the_oracle(oracle, emul, P, name, k):
    """All seven arrays, bit for bit; the seeds the emulation's d_reseed gives in iteration k are the census's; and refine leaves the emulation's frame as it was."""
    want = RC.oracle_refine(oracle, P, name, k)
    got = RC.emul_refine(emul, P, name, k)
    print(RC.census_line(oracle, emul, P, name) if k == RC.CASE[name].ks[0] else "")
    assert RC.refine_mismatch(want, got.arrays) is None, (name, k)
    assert np.array_equal(RC.reseed_census(oracle, P, name, k).seeds, got.seeds[k - 1]), (name, k)
    r = RC.oracle_run(oracle, P, name)
    assert C.emul_equals_oracle(RC.emul_run(emul, P, name), r.labels, r.h) is None


def test_refine_zero_is_the_extract_state(oracle, emul, P):
    for name in ("d-deep-chain-cold", "g-seed-ghosts-one-sweep"):
        r = RC.oracle_run(oracle, P, name)
        want = RC.oracle_refine(oracle, P, name, 0)
        assert RC.refine_mismatch(want, RC.emul_refine(emul, P, name, 0).arrays) is None
        assert np.array_equal(want["voxel_label"], r.h.get("VOXEL_SVLABEL")) and np.array_equal(want["label"], r.h.get("SV_LABELS"))


@pytest.mark.parametrize("name", RC.NAMES)
def test_the_census_table_in_the_docstring_is_the_census(oracle, emul, P, name):
    line = RC.census_line(oracle, emul, P, name)
    assert line in RC.__doc__.splitlines(), line
