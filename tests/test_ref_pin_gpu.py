"""The HIP merge loop and the scorer against the REFERENCE'S OWN code (oracle/_ref/libf3ds_ref.so: the reference's clustering, clustering_state, testing and
color_utilities sources compiled unchanged, tests/ref_pin_common.py), on the cases tests/test_ref_pin_cpu.py compares with the oracle.

Nothing outside the tree is read: the library was built where a checkout of the reference was at hand and travelled here with the tree; without it the tests fail.

For every case whose (survivor, absorbed) sequence is the same in the reference and in both oracles (all of them at the time of writing; at least three quarters have to
be) Context.cluster_supervoxels equals the reference exactly on region_of_sv, the voxel labels, the two label columns of merge_tree(), n_merges, n_regions and
region_adjacency(); the merge weights and lambda lie within the bound test_ref_pin_cpu.py asserts between the reference (libm) and the default oracle (csrc/f3ds_math.h),
twice what was measured (ref_pin_common.BOUND); evaluate() of a whole frame equals the reference's Testing on the device's supervoxels.  Mass ties and NaN cases are
compared on labels.  Where the reference throws, the device answers with the code the exception maps to -- except a pair listed twice and a self-pair, which the device
refuses up front with ERR_ARG as include/f3ds.h documents (the reference throws std::out_of_range once it meets the pair a second time, or not at all)."""
import numpy as np
import pytest

import ref_pin_common as R
from golden_cases import case_params, case_points, synthetic_truth

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in R.CASES]
LAYOUTS = [dict(F3DS_MERGE_NW=nw, F3DS_MERGE_KEYS=k) for nw in ("4", "8") for k in ("lds", "global")] + [dict(F3DS_FORCE_GLOBAL_MERGE="1")]


@pytest.fixture(scope="module")
def ref():
    chk, why = R.load_ref()
    if chk is None:
        pytest.fail(why + " (it is built by `make -C oracle` where the reference checkout is and travels with the tree)")
    return chk


@pytest.fixture(scope="module")
def ctx(P):
    if P.device_count() < 1:
        pytest.fail("GPU test selected but libf3ds sees no HIP device (no CPU fallback exists)")
    c = P.Context(0)
    yield c
    c.close()


def comparable(ref, oracle, oracle_libm, P, name):
    r = R.case_run("ref", ref, P, name)
    return r, R.same_sequence(r, R.case_run("math", oracle, P, name)) and R.same_sequence(r, R.case_run("libm", oracle_libm, P, name))


def check_against_the_reference(context, region, vlab, r, what):
    assert np.array_equal(region, r.region) and np.array_equal(vlab, r.vlab), what
    surv, absorbed, w = context.merge_tree()
    assert np.array_equal(np.stack([surv, absorbed], axis=1), r.merges[:, :2]), what
    assert (context.result.n_merges, context.result.n_regions) == (len(r.merges), len(r.regions["label"])), what
    assert np.array_equal(context.region_adjacency(), r.radj), what
    dw = R.rel_diff(w, r.merges[:, 2].view(np.float32)); dl = R.rel_diff([np.float32(context.result.lambda_)], [r.lam])
    assert dw <= R.BOUND["weight"] and dl <= R.BOUND["lambda_"], (what, dw, dl)
    assert np.isnan(np.float32(context.result.lambda_)) == np.isnan(r.lam)
    g = context.regions()                                       # the regions the device reports are the reference's: same keys, same sizes
    assert np.array_equal(g["label"], r.regions["label"]) and np.array_equal(g["n_voxels"], r.regions["n_voxels"]), what


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_reference(ref, oracle, oracle_libm, P, ctx, name):
    c = R.CASE[name]
    sv, pairs = R.graph(name)
    prm = R.params(P, c)
    if c.kind == "throws":
        r = R.case_run("ref", ref, P, name)
        want = c.expect if c.oracle_expect is None else c.oracle_expect
        assert c.expect is None or r.rc == c.expect
        if want == P.ERR_OUT_OF_RANGE:
            with pytest.raises(IndexError):
                ctx.cluster_supervoxels(sv, pairs, prm)
        else:
            with pytest.raises(P.F3dsError) as e:
                ctx.cluster_supervoxels(sv, pairs, prm)
            assert e.value.code == want, (name, e.value.code)
        return
    r, same = comparable(ref, oracle, oracle_libm, P, name)
    region, vlab = ctx.cluster_supervoxels(sv, pairs, prm)
    if c.kind == "tie":
        assert np.array_equal(region, r.region) and np.array_equal(vlab, r.vlab), name
        assert (ctx.result.n_merges, ctx.result.n_regions) == (len(r.merges), len(r.regions["label"]))
        return
    if not same:                # (the default oracle's sequence differs from the reference's by the libm distance: such a case is not compared; test_enough_cases_are_compared counts them)
        return
    check_against_the_reference(ctx, region, vlab, r, name)


def test_enough_cases_are_compared(ref, oracle, oracle_libm, P):
    runs = [comparable(ref, oracle, oracle_libm, P, c.name)[1] for c in R.CASES if c.kind == "run"]
    assert sum(runs) >= R.SAME_SEQUENCE_SHARE * len(runs), (sum(runs), len(runs))


@pytest.mark.parametrize("env", LAYOUTS, ids=lambda v: "-".join("%s" % x for x in v.values()))
def test_largest_case_in_every_merge_kernel_layout(ref, oracle, oracle_libm, P, ctx, monkeypatch, env):
    """The largest case (320 supervoxels) with 4 and 8 waves, keys in LDS and in global memory, and through the all-global d_merge."""
    name = R.LARGEST
    r, same = comparable(ref, oracle, oracle_libm, P, name)
    assert same and len(R.graph(name)[0]["label"]) == max(len(R.graph(c.name)[0]["label"]) for c in R.CASES)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sv, pairs = R.graph(name)
    region, vlab = ctx.cluster_supervoxels(sv, pairs, R.params(P, R.CASE[name]))
    assert ctx.merge_layout() == ((0, 0) if "F3DS_FORCE_GLOBAL_MERGE" in env else (int(env["F3DS_MERGE_NW"]), 2 if env["F3DS_MERGE_KEYS"] == "lds" else 0))
    check_against_the_reference(ctx, region, vlab, r, "%s under %s" % (name, env))


@pytest.mark.parametrize("name", ["fixture_launch_flags", "rgbd_160x120"])
def test_device_frame_equals_the_reference_on_its_supervoxels(ref, oracle, P, ctx, name):
    """A whole frame on the device (the fixture at --CVX --AL -t 0.2: 597 supervoxels; a synthetic RGB-D frame: 327) against the reference run on the supervoxel map +
    adjacency the default oracle's VCCS half exports for it (what main() hands to set_initialstate; the device's supervoxels equal them bit for bit, test_gpu_parity.py):
    per-point labels, merge sequence, counts, region adjacency, weights and lambda within the bound, and evaluate() = Testing(get_labeled_cloud(), truth)."""
    pts, prm = case_points(P, name), case_params(P, name)
    rc, olabels, ores, h = oracle.segment(pts, prm)
    assert rc == 0
    sv, pairs = h.export_supervoxels()
    r = R.run(ref, sv, pairs, prm, True)
    assert r.rc == 0 and np.array_equal(r.merges[:, :2], h.get("MERGES").reshape(-1, 3)[:, :2]), "the default oracle's sequence differs from the reference's on this frame"
    labels = ctx.segment(pts, prm)
    surv, absorbed, w = ctx.merge_tree()
    assert np.array_equal(np.stack([surv, absorbed], axis=1), r.merges[:, :2])
    assert (ctx.result.n_merges, ctx.result.n_regions, ctx.result.n_supervoxels) == (len(r.merges), len(r.regions["label"]), len(sv["label"]))
    assert np.array_equal(ctx.region_adjacency(), r.radj)
    assert R.rel_diff(w, r.merges[:, 2].view(np.float32)) <= R.BOUND["weight"] and R.rel_diff([np.float32(ctx.result.lambda_)], [r.lam]) <= R.BOUND["lambda_"]
    # per point: the reference's label of the voxel's OWNING supervoxel (a ghost leaf also sits in another supervoxel's list: the owner's label is written last by none of
    # the two sides in particular, so such voxels are left out), NO_LABEL outside every voxel
    pv = h.get("POINT_VOXEL"); own = h.get("VOXEL_SVLABEL")
    row_sv = np.repeat(sv["label"], np.diff(sv["voxel_offset"]).astype(np.int64))
    owned = row_sv == own[sv["voxel_leaf"]]
    by_leaf = np.full(len(own), 0xFFFFFFFF, np.uint32)
    by_leaf[sv["voxel_leaf"][owned]] = r.vlab[owned]
    inside = pv >= 0
    want = np.full(len(pts), 0xFFFFFFFF, np.uint32); want[inside] = by_leaf[pv[inside]]
    assert np.array_equal(labels, want) and np.array_equal(labels, olabels)
    truth = synthetic_truth(pts)
    txyz, tlab = R.truth_cloud(oracle, h, truth)
    R.set_truth_points(ref, r.h, txyz)
    rc, pr = r.h.evaluate(tlab)
    got = R.perf_array(ctx.evaluate(truth))
    assert rc == 0 and R.rel_diff(got, R.perf_array(pr)) <= R.BOUND["perf"], (got, R.perf_array(pr))
