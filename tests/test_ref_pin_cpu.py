"""The oracle's merge half and scorer against the REFERENCE'S OWN code: src/clustering.cpp, clustering_state.cpp, testing.cpp and color_utilities.cpp of the reference
checkout, compiled unchanged against oracle/ref_shim into oracle/_ref/libf3ds_ref.so and driven through oracle/ref_driver.cpp (tests/ref_pin_common.py).

Against libf3ds_oracle_libm.so -- the same restatement on libm, as the reference is -- the comparison is BIT FOR BIT (a NaN equals a NaN, nothing else is relaxed):
region of every supervoxel, voxel labels, the merge sequence with its weight bits, lambda, regions() (label, voxel count, centroid, normal, mean colour), the region
adjacency, the labelled cloud and all seven Performance fields; error codes where the reference throws.  What both sides share stays unpinned: computeCentroid,
computePointNormal / eigen33, flipNormalTowardsViewpoint and cvtColor are the oracle's own functions on both sides.

Against the default oracle (csrc/f3ds_math.h instead of libm, the one the device is bit-equal to) the distance is measured and bounded by twice what was measured here.

Where the reference and the oracle answer differently on purpose (both refuse, with different codes) the test says so: a pair listed twice or a self-pair is ERR_ARG
up front in the oracle and on the device (include/f3ds.h); the reference runs and throws std::out_of_range from map::at in merge() once it meets the pair a second
time (src/clustering.cpp:441) -- or never, when that pair is never merged.  An empty label cloud is std::invalid_argument in the reference (testing.cpp:414,431),
which the driver maps to ERR_RANGE like the reference's other invalid_argument; the oracle's eval_clouds entry answers ERR_ARG."""
import numpy as np
import pytest

import devprobe_inputs as D
import ref_pin_common as R
from conftest import first_mismatch, same_bits
from golden_cases import case_params, case_points, synthetic_truth

NAMES = [c.name for c in R.CASES]
BOUND, SAME_SEQUENCE_SHARE = R.BOUND, R.SAME_SEQUENCE_SHARE


@pytest.fixture(scope="module")
def ref():
    chk, why = R.load_ref()
    if chk is None:
        if R.reference_present():
            pytest.fail(why)
        pytest.skip(why)
    return chk


def assert_same_run(r, o, what):
    """Everything a run leaves behind, bit for bit (NaN = NaN)."""
    assert (r.rc, o.rc) == (0, 0), what
    assert np.array_equal(r.region, o.region) and np.array_equal(r.vlab, o.vlab), what
    assert first_mismatch("MERGES", r.merges, o.merges) is None, what
    assert same_bits(np.array([r.lam]), np.array([o.lam])), (what, r.lam, o.lam)
    assert (r.res.n_merges, r.res.n_regions) == (o.res.n_merges, o.res.n_regions) == (len(o.merges), len(o.regions["label"])), what
    assert sorted(r.regions) == sorted(o.regions)
    for k in o.regions:
        assert first_mismatch("regions." + k, r.regions[k], o.regions[k]) is None, what
    assert np.array_equal(r.radj, o.radj), what
    assert same_bits(r.cloud[0], o.cloud[0]) and np.array_equal(r.cloud[1], o.cloud[1]), what
    for a, b in zip(r.h.region_voxels(), o.h.region_voxels()):
        assert same_bits(a, b), what
    assert same_bits(r.perf, o.perf), (what, r.perf, o.perf)


# ------------------------------------------------------------------------------------------------ the merge half
@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_the_libm_oracle(ref, oracle_libm, P, name):
    c = R.CASE[name]
    sv, pairs = R.graph(name)
    assert np.diff(sv["voxel_offset"]).min() >= 4 and len(sv["label"]) <= 320, "every supervoxel holds at least 4 voxels (fewer give a degenerate PCA normal after the first merge)"
    r = R.case_run("ref", ref, P, name); o = R.case_run("libm", oracle_libm, P, name)
    if c.kind == "throws":
        if c.expect is not None:
            assert r.rc == c.expect, (name, r.rc)
        else:                   # a self-pair: a NaN weight in the reference's multimap, whose place in the order the C++ standard leaves open; the run ends, with or without map::at throwing
            assert r.rc in (0, P.ERR_OUT_OF_RANGE), (name, r.rc)
        assert o.rc == (c.expect if c.oracle_expect is None else c.oracle_expect), (name, o.rc)
        return
    assert_same_run(r, o, name)
    rc, p = r.h.evaluate(R.truth_of(sv))            # Testing(get_labeled_cloud(), truth) on the handle = Testing on the two clouds
    assert rc == 0 and same_bits(R.perf_array(p), r.perf)


def test_every_class_of_input_is_populated(ref, oracle_libm, P):
    """REQUIRED of ref_pin_common.py: merge criteria and metrics, the EQ clamp and throw, the adaptive-lambda degenerates, the adjacency input forms, every rewrite
    branch of merge(), ties at the head of the map and the threshold edges -- each shown on the libm oracle's own data of at least one case."""
    have = {}
    for c in R.CASES:
        sv, pairs = R.graph(c.name)
        o = R.case_run("libm", oracle_libm, P, c.name)
        twin = None
        if c.kind == "throws" and c.expect == P.ERR_EQ_BIN:       # the same graph under a criterion that does not throw shows the delta_g that makes t_g throw
            t = R.run(oracle_libm, sv, pairs, P.default_params(color_metric=c.prm["color_metric"], merging=R.ADAPTIVE, threshold=0.0), False)
            twin = float(t.h.get("EDGE_DELTAS").reshape(-1, 2)[:, 1].max())
        for k in R.classes(c, sv, pairs, R.params(P, c), o, twin):
            have.setdefault(k, []).append(c.name)
    missing = [k for k in R.REQUIRED if k not in have]
    assert not missing, missing


def test_cluster_again_with_other_thresholds_on_one_object(ref, oracle_libm, P):
    """cluster(t) on an object that already has its initial weights (src/clustering.cpp:675-678): a larger t, a smaller t, t = 0, t above every weight, and t equal to a
    logged weight (the loop's test is `<`: it stops AT that merge)."""
    sv, pairs = R.graph("scene10x10-to-the-end")
    prm = P.default_params(merging=R.MANUAL, threshold=0.2)
    r = R.run(ref, sv, pairs, prm, True); o = R.run(oracle_libm, sv, pairs, prm, False)
    assert_same_run(r, o, "first")
    full = R.case_run("libm", oracle_libm, P, "scene10x10-to-the-end").merges
    w = full[:, 2].view(np.float32)
    k_eq = 20
    assert (w[:k_eq] < w[k_eq]).all()                                    # (a weight no earlier merge reaches: the run at t = w[k_eq] ends before merge k_eq)
    counts = {}
    for what, t in (("larger", 0.3), ("smaller", 0.15), ("zero", 0.0), ("above", 5.0), ("equal", float(w[k_eq])), ("first again", 0.2)):
        p2 = prm.copy(); p2.threshold = t
        rc1, vr, rr = r.h.cluster(p2, len(sv["voxel_rgba"])); rc2, _, ro = o.h.cluster(p2, 0)
        assert (rc1, rc2) == (0, 0)
        mr, mo = r.h.get("MERGES").reshape(-1, 3), o.h.get("MERGES").reshape(-1, 3)
        assert first_mismatch("MERGES at " + what, mr, mo) is None and (rr.n_merges, rr.n_regions) == (ro.n_merges, ro.n_regions) == (len(mo), len(sv["label"]) - len(mo))
        assert np.array_equal(mo, full[:len(mo)])                      # every run is a prefix of the run to the end
        stop = np.nonzero(~(w < np.float32(t)))[0]
        assert len(mo) == (int(stop[0]) if len(stop) else len(w)), what
        _, lab, _ = o.h.voxel_cloud(); _, _, idx = o.h.region_voxels()
        want = np.zeros(len(vr), np.uint32); want[idx] = lab
        assert np.array_equal(vr, want), what
        for a, b in zip(r.h.voxel_cloud()[:2], o.h.voxel_cloud()[:2]):
            assert same_bits(a, b), what
        counts[what] = len(mo)
    assert counts["zero"] == 0 < counts["smaller"] < len(r.merges) == counts["first again"] < counts["larger"] < counts["above"] == len(full) and counts["equal"] == k_eq, counts


# ------------------------------------------------------------------------------------------------ frames: the fixture, all_thresh / best_thresh
_frames = {}


def frame(chk, P, which, name):
    """A frame through an oracle's VCCS half: its supervoxel map + adjacency (what main() hands to set_initialstate) and the truth cloud main() makes."""
    if (which, name) not in _frames:
        pts, prm = case_points(P, name), case_params(P, name)
        rc, labels, res, h = chk.segment(pts, prm)
        assert rc == 0
        sv, pairs = h.export_supervoxels()
        truth = synthetic_truth(pts)
        txyz, tlab = R.truth_cloud(chk, h, truth)
        _frames[(which, name)] = dict(pts=pts, prm=prm, h=h, res=res, sv=sv, pairs=pairs, truth=truth, txyz=txyz, tlab=tlab)
    return _frames[(which, name)]


@pytest.mark.parametrize("name", ["fixture_launch_flags", "rgbd_160x120"])
def test_reference_on_a_frames_supervoxels(ref, oracle_libm, P, name):
    """The fixture's 597 supervoxels (--CVX --AL -t 0.2, whole: the reference takes half a second) and a synthetic RGB-D frame's, as the libm oracle's VCCS half exports
    them: the reference's merges, labels and scores equal the oracle's own whole-frame run."""
    f = frame(oracle_libm, P, "libm", name)
    r = R.run(ref, f["sv"], f["pairs"], f["prm"], True); o = R.run(oracle_libm, f["sv"], f["pairs"], f["prm"], False)
    assert_same_run(r, o, name)
    assert name != "fixture_launch_flags" or len(f["sv"]["label"]) == 597
    assert first_mismatch("MERGES", r.merges, f["h"].get("MERGES").reshape(-1, 3)) is None and len(r.merges) > 100
    R.set_truth_points(ref, r.h, f["txyz"])
    rc1, pr = r.h.evaluate(f["tlab"]); rc2, po = f["h"].evaluate(f["truth"])
    assert (rc1, rc2) == (0, 0) and same_bits(R.perf_array(pr), R.perf_array(po)), (R.perf_array(pr), R.perf_array(po))
    assert len(f["txyz"]) >= len(f["sv"]["voxel_rgba"])                 # (the truth cloud also holds the voxels no supervoxel owns)


SWEEPS = {"start > end": (0.3, 0.1, 0.03), "step does not divide the range": (0.1, 0.3, 0.07), "one threshold": (0.2, 0.2, 0.5), "ends at 1": (0.9, 1.0, 0.05)}


@pytest.mark.parametrize("what", sorted(SWEEPS))
def test_all_thresh_and_best_thresh(ref, oracle_libm, P, what):
    """all_thresh + best_thresh + cluster(best) (src/clustering.cpp:691-774) on a frame of 327 supervoxels: the thresholds visited (float accumulation of the step), the
    seven scores at each, the best threshold and the state the object is left in."""
    f = frame(oracle_libm, P, "libm", "rgbd_160x120")
    r = R.run(ref, f["sv"], f["pairs"], f["prm"], True)
    R.set_truth_points(ref, r.h, f["txyz"])
    s, e, st = SWEEPS[what]
    rc1, bt1, bp1, tab1, vlab = r.h.auto_threshold(f["prm"], f["tlab"], len(f["sv"]["voxel_rgba"]), s, e, st)
    rc2, bt2, bp2, tab2, plab = f["h"].auto_threshold(f["prm"], f["truth"], len(f["pts"]), s, e, st)
    assert (rc1, rc2) == (0, 0)
    assert list(tab1) == list(tab2) and len(tab1) == {"start > end": 7, "step does not divide the range": 3, "one threshold": 1, "ends at 1": 3}[what], list(tab1)
    for t in tab1:
        assert same_bits(np.array([tab1[t][k] for k in R.PERF], np.float32), np.array([tab2[t][k] for k in R.PERF], np.float32)), (t, tab1[t], tab2[t])
    assert np.float32(bt1) == np.float32(bt2) and same_bits(R.perf_array(bp1), R.perf_array(bp2)) and bp1.fscore > 0
    assert first_mismatch("MERGES", r.h.get("MERGES"), f["h"].get("MERGES")) is None
    _, lab, _ = f["h"].voxel_cloud()
    assert same_bits(r.h.voxel_cloud()[0], f["h"].voxel_cloud()[0]) and np.array_equal(r.h.voxel_cloud()[1], lab)
    assert np.array_equal(vlab[r.h.region_voxels()[2]], lab)             # one label per input voxel = the labelled cloud's, through the voxel index


def test_all_thresh_bounds_out_of_range(ref, oracle_libm, P):
    f = frame(oracle_libm, P, "libm", "rgbd_160x120")
    r = R.run(ref, f["sv"], f["pairs"], f["prm"], True)
    R.set_truth_points(ref, r.h, f["txyz"])
    for s, e, st in ((-0.1, 0.5, 0.1), (0.1, 1.5, 0.1), (0.1, 0.5, 2.0), (0.1, 0.5, -0.1), (1.01, 0.5, 0.1)):
        assert r.h.auto_threshold(f["prm"], f["tlab"], len(f["sv"]["voxel_rgba"]), s, e, st)[0] == P.ERR_OUT_OF_RANGE, (s, e, st)      # std::out_of_range (:694-698)
        assert f["h"].auto_threshold(f["prm"], f["truth"], len(f["pts"]), s, e, st)[0] == P.ERR_OUT_OF_RANGE, (s, e, st)
    # a zero step never ends in the reference; the driver, the oracle and the device refuse it
    assert r.h.auto_threshold(f["prm"], f["tlab"], len(f["sv"]["voxel_rgba"]), 0.1, 0.5, 0.0)[0] == P.ERR_OUT_OF_RANGE
    assert f["h"].auto_threshold(f["prm"], f["truth"], len(f["pts"]), 0.1, 0.5, 0.0)[0] == P.ERR_OUT_OF_RANGE


def test_best_thresh_with_every_fscore_zero(ref, P):
    """A truth cloud that shares no point with the segmentation: every intersection is 0, the first truth segment is matched with row 0 (maxCoeff of a zero column), every
    other finds row 0 taken and nothing else (-1); precision = recall = 0, the F-score is set to 0 (testing.cpp:292-295).  best_thresh then keeps its initial
    (0, all-zero scores) (clustering.cpp:761-773) and main() clusters at 0: nothing is merged.  The oracle's and the device's all_thresh take their truth cloud from the
    frame's own voxels and cannot be brought here; their best_thresh is the same three lines."""
    sv, pairs = R.graph("scene6x6-both-directions")
    prm = R.params(P, R.CASE["scene6x6-both-directions"])
    r = R.run(ref, sv, pairs, prm, True)
    assert len(r.merges) > 5
    R.set_truth_points(ref, r.h, sv["voxel_xyz"] + np.float32(100.0))
    rc, bt, bp, tab, vlab = r.h.auto_threshold(prm, R.truth_of(sv), len(sv["voxel_rgba"]), 0.1, 0.3, 0.05)
    assert rc == 0 and len(tab) >= 4 and all(v["fscore"] == 0 and v["precision"] == 0 and v["recall"] == 0 and v["fnr"] == 1 for v in tab.values()), tab
    assert bt == 0.0 and not R.perf_array(bp).any()
    assert len(r.h.get("MERGES")) == 0 and np.array_equal(vlab, np.repeat(np.arange(len(sv["label"]), dtype=np.uint32), np.diff(sv["voxel_offset"])))


# ------------------------------------------------------------------------------------------------ the scorer on label clouds built by hand
def _grid(n):
    return np.stack([np.arange(n, dtype=np.float32), (np.arange(n) % 3).astype(np.float32), np.zeros(n, np.float32)], axis=1)


def _scorer_cases():
    g = _grid(12)
    out = {}
    # name -> (segm xyz, segm labels, truth xyz, truth labels, known answers {field: value} or None)
    # truth segments of 4, 4 and 4 points: t_sizes (keyed by size) keeps the first only, the other two are never matched (fnr = 8 / 12, recall = 4 / 12)
    out["truth segments of equal size"] = (g, np.repeat([0, 1, 2], 4), g, np.repeat([5, 6, 7], 4), dict(recall=4 / 12, fnr=8 / 12, precision=4 / 12, fpr=0.0))
    # one segment against truth segments of 8 and 4: the larger takes row 0, the smaller finds it taken and no other row with an intersection: -1
    out["best row taken, then -1"] = (g, np.zeros(12), g, np.repeat([0, 1], [8, 4]), dict(recall=8 / 12, fnr=4 / 12, fpr=4 / 12, precision=np.float32(8 * 8) / np.float32(12) / np.float32(12)))
    # truth A (7 points) and B (5): both have their largest intersection with segment 0; B retries and gets segment 1 (2 points)
    out["best row taken, retry finds another"] = (g, np.repeat([0, 1], [10, 2]), g, np.array([0] * 7 + [1] * 5), dict(recall=9 / 12))
    # a column with the same intersection in two rows: maxCoeff gives the first
    out["tie in maxCoeff"] = (g, np.repeat([0, 1, 2], [4, 4, 4]), g, np.repeat([0, 1], [8, 4]), dict(recall=8 / 12))
    out["more truth than segmentation segments"] = (g, np.repeat([0, 1], [6, 6]), g, np.repeat([0, 1, 2, 3], [5, 4, 2, 1]), None)
    out["more segmentation than truth segments"] = (g, np.repeat([0, 1, 2, 3], [5, 4, 2, 1]), g, np.repeat([0, 1], [7, 5]), None)
    out["a point in only one cloud"] = (g[:10], np.repeat([0, 1], [5, 5]), g[2:], np.repeat([0, 1], [6, 4]), None)
    rep = np.vstack([g, g[:4], g[:2]])
    out["repeated points"] = (rep, np.concatenate([np.repeat([0, 1], [6, 6]), [0, 0, 1, 1], [1, 0]]), np.vstack([g, g[3:6]]), np.concatenate([np.repeat([0, 1, 2], [3, 4, 5]), [2, 2, 0]]), None)
    out["one segment on either side"] = (g, np.full(12, 9), g, np.full(12, 4), dict(voi=0.0, precision=1.0, recall=1.0, fscore=1.0, wov=1.0, fpr=0.0, fnr=0.0))
    out["one segment against many"] = (g, np.arange(12), g, np.zeros(12), None)
    out["labels that skip values, unsorted points"] = (g[::-1], np.repeat([70000, 3, 900], 4), g, np.repeat([4000000000, 17], [5, 7]), None)
    rng = np.random.default_rng(77)
    for i in range(24):        # random label clouds on a shared lattice with drop-outs and repeats on both sides
        n = int(rng.integers(20, 90)); base = _grid(n)
        a = rng.integers(0, n, int(n * rng.uniform(0.6, 1.4))); b = rng.integers(0, n, int(n * rng.uniform(0.6, 1.4)))
        la = rng.integers(0, int(rng.integers(1, 7)), n)[a]; lb = (rng.integers(0, int(rng.integers(1, 7)), n) // (1 + i % 2))[b]
        out["random %d" % i] = (base[a], la, base[b], lb, None)
    return out


SCORER = _scorer_cases()


@pytest.mark.parametrize("what", sorted(SCORER))
def test_scorer_on_label_clouds(ref, oracle_libm, oracle, P, what):
    sx, sl, tx, tl, known = SCORER[what]
    rc1, pr = R.eval_clouds(ref, sx, sl, tx, tl); rc2, po = R.eval_clouds(oracle_libm, sx, sl, tx, tl); rc3, pm = R.eval_clouds(oracle, sx, sl, tx, tl)
    assert (rc1, rc2, rc3) == (0, 0, 0)
    assert same_bits(pr, po) and same_bits(pr, pm), (what, pr, po, pm)
    for k, v in (known or {}).items():                # the branch the case is for was taken: its known answer, to float rounding
        assert abs(float(pr[R.PERF.index(k)]) - float(v)) <= 4 * np.finfo(np.float32).eps, (what, k, pr, v)


def test_scorer_refuses_an_empty_cloud(ref, oracle_libm, P):
    g = _grid(6); lab = np.repeat([0, 1], 3); none = np.zeros((0, 3), np.float32); nol = np.zeros(0, np.uint32)
    for sx, sl, tx, tl in ((none, nol, g, lab), (g, lab, none, nol), (none, nol, none, nol)):
        assert R.eval_clouds(ref, sx, sl, tx, tl)[0] == P.ERR_RANGE          # std::invalid_argument (testing.cpp:414-416, 431-433), as ref_driver.cpp maps it
        assert R.eval_clouds(oracle_libm, sx, sl, tx, tl)[0] == P.ERR_ARG    # the oracle's entry refuses it as a bad argument


# ------------------------------------------------------------------------------------------------ per element
N_ROWS = 200000


def test_ciede2000_rows(ref, oracle_libm, cases):
    """lab_ciede00 on 200 000 seeded random Lab pairs (the whole gamut, near-equal colours, greys) and on every row of the device probe's case (the reference's 34 known
    answers in both orders, hue branches, exact-zero chroma, NaN / Inf / -0 specials)."""
    rng = np.random.default_rng(5)
    lab = np.stack([rng.uniform(0, 100, 2 * N_ROWS), rng.uniform(-110, 110, 2 * N_ROWS), rng.uniform(-110, 110, 2 * N_ROWS)], axis=1).astype(np.float32).reshape(N_ROWS, 6)
    near = rng.random(N_ROWS) < 0.3
    lab[near, 3:] = lab[near, :3] + rng.normal(0, 1.5, (int(near.sum()), 3)).astype(np.float32)
    grey = rng.random(N_ROWS) < 0.05
    lab[grey, 1:3] = 0
    special = cases("n_ciede00").rows[:, :6].view(np.float32)
    assert len(special) > 4000 and np.isnan(special).any() and np.isinf(special).any()
    for rows in (lab, special):
        a, b = R.rows(ref, "ciede00", rows), R.rows(oracle_libm, "ciede00", rows)
        assert same_bits(a, b), first_mismatch("ciede00", a, b)


def test_rgb_eucl_rows(ref, oracle_libm, cases):
    rng = np.random.default_rng(6)
    rgb = rng.uniform(0, 255, (N_ROWS, 6)).astype(np.float32)
    whole = rng.random(N_ROWS) < 0.5
    rgb[whole] = np.round(rgb[whole])
    special = cases("n_rgb_eucl").rows[:, :6].view(np.float32)
    for rows in (rgb, special):
        a, b = R.rows(ref, "rgb_eucl", rows), R.rows(oracle_libm, "rgb_eucl", rows)
        assert same_bits(a, b), first_mismatch("rgb_eucl", a, b)


def test_mean_color_rows(ref, oracle_libm):
    """mean_color's running mean over voxel lists of 1 .. 60 colours (and a few of thousands), 200 000 lists."""
    rng = np.random.default_rng(7)
    cnt = rng.integers(1, 61, N_ROWS); cnt[:20] = rng.integers(2000, 9000, 20)
    off = np.zeros(N_ROWS + 1, np.uint32); off[1:] = np.cumsum(cnt)
    rgba = rng.integers(0, 1 << 24, int(off[-1])).astype(np.uint32)
    flat = rng.random(N_ROWS) < 0.2                                   # lists of one colour, and of two neighbouring colours
    owner = np.repeat(np.arange(N_ROWS), cnt)
    first = rgba[off[:-1].astype(np.int64)]
    rgba[flat[owner]] = (first[owner] ^ (rng.integers(0, 2, len(owner)).astype(np.uint32) * (owner % 3 == 0)))[flat[owner]]
    a, b = R.mean_color_rows(ref, rgba, off), R.mean_color_rows(oracle_libm, rgba, off)
    assert same_bits(a, b), first_mismatch("mean_color", a, b)


@pytest.fixture(scope="module")
def cases():
    return lambda name: D.case(name)


# ------------------------------------------------------------------------------------------------ the distance to the default oracle
def test_distance_to_the_default_oracle(ref, oracle, oracle_libm, P, capsys):
    """The default oracle (csrc/f3ds_math.h, what the device equals bit for bit) against the reference on every case: at least three quarters of the cases that are neither
    a mass tie nor NaN give the same (survivor, absorbed) sequence in the reference and in BOTH oracles; over those the merge weights, lambda and the seven scores differ
    by no more than BOUND.  Mass ties and NaN cases are compared on labels only."""
    worst = dict(weight=0.0, lambda_=0.0, perf=0.0); same, total, where = 0, 0, {}
    runs = [(c.name, c.kind, R.case_run("ref", ref, P, c.name), R.case_run("math", oracle, P, c.name), R.case_run("libm", oracle_libm, P, c.name)) for c in R.CASES if c.kind != "throws"]
    for name in ("fixture_launch_flags", "rgbd_160x120"):          # the reference on the DEFAULT oracle's supervoxels (the device's), against the default oracle
        f = frame(oracle, P, "math", name)
        runs.append((name, "run", R.run(ref, f["sv"], f["pairs"], f["prm"], True), R.run(oracle, f["sv"], f["pairs"], f["prm"], False), None))
    for name, kind, r, m, o in runs:
        if kind == "tie":
            assert np.array_equal(r.region, m.region) and np.array_equal(r.vlab, m.vlab), name
            continue
        total += 1
        if not (R.same_sequence(r, m) and (o is None or R.same_sequence(r, o))):
            continue
        same += 1
        assert np.array_equal(r.region, m.region) and np.array_equal(r.vlab, m.vlab) and np.array_equal(r.radj, m.radj), name
        d = dict(weight=R.rel_diff(r.merges[:, 2].view(np.float32), m.merges[:, 2].view(np.float32)), lambda_=R.rel_diff([r.lam], [m.lam]), perf=R.rel_diff(r.perf, m.perf))
        for k in d:
            if d[k] > worst[k]:
                worst[k], where[k] = d[k], name
    with capsys.disabled():
        print("\nreference vs default oracle: same sequence in %d of %d cases; largest relative difference: %s" % (same, total, ", ".join("%s %.3g (%s)" % (k, worst[k], where.get(k, "-")) for k in worst)))
    assert same >= SAME_SEQUENCE_SHARE * total, (same, total)
    for k in worst:
        assert worst[k] <= BOUND[k], (k, worst[k], where.get(k))
