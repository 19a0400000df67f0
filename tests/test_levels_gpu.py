"""Hierarchy levels on the MI355X (f3ds_labels_at_thresholds, csrc/f3ds_levels.inc): every level is bit-equal to f3ds_recluster at its
threshold and to the oracle's cluster(t), in both table forms and in batches; the call leaves the context's state alone; the merge tree is
the merge log in the caller's labels; the CLI's --levels files equal separate -t runs."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, FIXTURE_PCD
from golden_cases import GOLDEN_CASES, case_points, case_params
from levels_common import level_thresholds

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "fast-3d-pointcloud-segmentation_amd", "supervoxel_clustering")
FORMS = [{}, {"F3DS_LEVELS_GLOBAL": "1"}, {"F3DS_LEVELS_GLOBAL": "1", "F3DS_RELABEL_LDS_CAP": "0"}]


def _at(prm, t):
    p = prm.copy()
    p.threshold = float(t)
    return p


def _levels_and_reclusters(ctx, pts, prm, ts):
    ctx.segment(pts, prm)
    got, nreg = ctx.labels_at_thresholds(ts)
    want = []
    for t in ts:
        lab = ctx.recluster(_at(prm, t))
        want.append((lab, int(ctx.result.n_regions), int(ctx.result.n_merges)))
    return got, nreg, want


_distinct = {}


def check_golden_levels(P, oracle, gpu_ctx, monkeypatch, name, after_segment=None):
    """Every level of a golden case equals recluster and the oracle's cluster(t), in every table form; returns the region counts of the levels.
    after_segment(ctx): called after every device call group (tests/test_narrow_launch_gpu.py asserts the launch shape there)."""
    pts, prm = case_points(P, name), case_params(P, name)
    rc, _, ores, h = oracle.segment(pts, prm)
    assert rc == 0
    ts = level_thresholds(h.get("MERGES").reshape(-1, 3)[:, 2].view(np.float32), prm.threshold)
    first = None
    for env in FORMS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got, nreg, want = _levels_and_reclusters(gpu_ctx, pts, prm, ts)
        if after_segment:
            after_segment(gpu_ctx)
        assert got.shape == (len(ts), len(pts))
        for l, (lab, nr, _) in enumerate(want):
            assert np.array_equal(got[l], lab), "%s %s: level %d (t = %r) differs from recluster" % (name, env, l, ts[l])
            assert nreg[l] == nr
        if first is None:
            first = (got.copy(), nreg.copy())
            for l, t in enumerate(ts):
                rc, olab, ores_t = h.cluster(_at(prm, t), len(pts))
                assert rc == 0 and np.array_equal(got[l], olab) and nreg[l] == ores_t.n_regions, "%s: level %d differs from the oracle" % (name, l)
        else:
            assert got.tobytes() == first[0].tobytes() and np.array_equal(nreg, first[1]), "%s: the table forms disagree (%s)" % (name, env)
        for k in env:
            monkeypatch.delenv(k)
    return first[1]


@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_golden_levels_equal_recluster_and_oracle(P, oracle, gpu_ctx, monkeypatch, name):
    nreg = check_golden_levels(P, oracle, gpu_ctx, monkeypatch, name)
    _distinct[name] = len(set(nreg.tolist()))


def test_most_golden_cases_have_three_region_counts():
    if len(_distinct) < len(GOLDEN_CASES):
        pytest.fail("run with the golden-case test above (it records the region counts)")
    assert sum(v >= 3 for v in _distinct.values()) >= len(_distinct) // 2 + 1, _distinct


def test_state_is_unchanged(P, gpu_ctx):
    name = "rgbd_320x240_ghosts"
    pts, prm = case_points(P, name), case_params(P, name)
    gpu_ctx.segment(pts, prm)
    before = dict(regions=gpu_ctx.regions(), cloud=gpu_ctx.voxel_cloud(), adj=gpu_ctx.region_adjacency(), vreg=gpu_ctx.debug("VOXEL_REGION"),
                  merges=gpu_ctx.debug("MERGES"), svreg=gpu_ctx.debug("SV_REGION"))
    res = (gpu_ctx.result.n_regions, gpu_ctx.result.n_merges)
    gpu_ctx.labels_at_thresholds([0.0, 0.05, 0.1, 0.2, 0.15])
    after = dict(regions=gpu_ctx.regions(), cloud=gpu_ctx.voxel_cloud(), adj=gpu_ctx.region_adjacency(), vreg=gpu_ctx.debug("VOXEL_REGION"),
                 merges=gpu_ctx.debug("MERGES"), svreg=gpu_ctx.debug("SV_REGION"))
    assert (gpu_ctx.result.n_regions, gpu_ctx.result.n_merges) == res
    for k in before:
        a, b = before[k], after[k]
        if isinstance(a, dict):
            assert a.keys() == b.keys() and all(np.asarray(a[x]).tobytes() == np.asarray(b[x]).tobytes() for x in a), k
        elif isinstance(a, tuple):
            assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b)), k
        else:
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), k
    later = gpu_ctx.recluster(_at(prm, 0.1))
    fresh = P.Context(0)
    try:
        fresh.segment(pts, prm)
        assert np.array_equal(later, fresh.recluster(_at(prm, 0.1)))
    finally:
        fresh.close()


def test_errors(P, gpu_ctx):
    fresh = P.Context(0)
    try:
        with pytest.raises(P.LogicError):
            fresh.labels_at_thresholds([0.1])
        with pytest.raises(P.LogicError):
            fresh.merge_tree()
        pts, prm = case_points(P, "rgbd_160x120"), case_params(P, "rgbd_160x120")
        fresh.segment(pts, prm)
        with pytest.raises(IndexError):
            fresh.labels_at_thresholds([0.1, np.nextafter(np.float32(prm.threshold), np.float32(1))])
        with pytest.raises(P.F3dsError) as e:
            fresh.labels_at_thresholds([0.1, float("nan")])
        assert e.value.code == -1
        lib = P.load_library()
        t = np.array([0.1], np.float32)
        assert lib.f3ds_labels_at_thresholds(fresh.handle, t.ctypes.data, 0, t.ctypes.data, 0, None) == -1
        assert lib.f3ds_labels_at_thresholds(fresh.handle, None, 1, t.ctypes.data, 0, None) == -1
        assert lib.f3ds_labels_at_thresholds(fresh.handle, t.ctypes.data, 1, None, 0, None) == -1
        fresh.recluster(_at(prm, 0.05))               # a recluster is a cluster run: T is now 0.05
        with pytest.raises(IndexError):
            fresh.labels_at_thresholds([0.1])
        fresh.labels_at_thresholds([0.05, 0.01])
        empty = np.full((100, 4), np.nan, np.float32)
        fresh.segment(empty, prm)                    # a frame without voxels: no cluster run
        with pytest.raises(P.LogicError):
            fresh.labels_at_thresholds([0.1])
    finally:
        fresh.close()


def _batch_frames(P):
    frames = []
    for name in sorted(GOLDEN_CASES):
        frames.append((case_points(P, name), case_params(P, name)))
    frames.append((P.synth_frame(0, 1000, 1000, 1000, 30), P.launch_params()))        # the bench workload's 1M-point frame
    frames.append((P.synth_frame(0, 21, 160, 120, 30), P.launch_params(voxel_res=0.02, seed_res=0.2)))
    frames.append((P.synth_frame(1, 5, 200, 150, 0), P.launch_params(voxel_res=0.03, seed_res=0.3, use_transform=0)))
    assert len(frames) == 16
    return frames


@pytest.mark.parametrize("env", FORMS[:2])
def test_batch_equals_single_calls(P, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    frames = _batch_frames(P)
    ts = np.array([0.2, 0.0, 0.05, 0.1, 0.15, 0.12, 0.18, 0.199], np.float32)          # (every golden run goes to T >= 0.2)
    ctxs = [P.Context(0) for _ in frames]
    try:
        for c, (pts, prm) in zip(ctxs, frames):
            c.segment(pts, prm)
        single = [c.labels_at_thresholds(ts) for c in ctxs]
        labels, nreg = P.labels_at_thresholds_batch(ctxs, ts)
        for i, (lab, nr) in enumerate(single):
            assert np.array_equal(labels[i], lab), "frame %d" % i
            assert np.array_equal(nreg[i], nr)
        assert np.array_equal(labels[13][0], ctxs[13].recluster(_at(frames[13][1], ts[0])))       # the 1M frame at T: its segmentation
        import torch
        outs = [torch.empty(len(ts) * len(f[0]), dtype=torch.int32, device="cuda") for f in frames]
        torch.cuda.synchronize()
        P.labels_at_thresholds_batch(ctxs, ts, out=outs, on_device=True)
        for i, o in enumerate(outs):
            assert np.array_equal(o.cpu().numpy().view(np.uint32).reshape(len(ts), -1), labels[i]), "device output, frame %d" % i
    finally:
        for c in ctxs:
            c.close()


def test_user_mode_levels_per_voxel(P, oracle, gpu_ctx):
    name = "rgbd_320x240_ghosts"
    pts, prm = case_points(P, name), case_params(P, name)
    rc, _, _, h = oracle.segment(pts, prm)
    assert rc == 0
    sv, pairs = h.export_supervoxels()
    sv = dict(sv)
    key = lambda a: (np.asarray(a, np.uint32) * 5 + 17).astype(np.uint32)      # caller keys that are not the internal handles
    sv["label"] = key(sv["label"])
    pairs = key(pairs)
    region, vlab = gpu_ctx.cluster_supervoxels(sv, pairs, prm)
    a, b, w = gpu_ctx.merge_tree()
    m = gpu_ctx.debug("MERGES").reshape(-1, 3)
    assert np.array_equal(a, m[:, 0]) and np.array_equal(b, m[:, 1]) and w.tobytes() == m[:, 2].tobytes()
    assert np.isin(a, sv["label"]).all() and np.isin(b, sv["label"]).all()
    ts = level_thresholds(w, prm.threshold)
    got, nreg = gpu_ctx.labels_at_thresholds(ts)
    assert got.shape == (len(ts), len(vlab))
    assert np.array_equal(got[-1], vlab)
    for l, t in enumerate(ts):
        lab = gpu_ctx.recluster(_at(prm, t))
        assert np.array_equal(got[l], lab), "level %d" % l
        assert nreg[l] == gpu_ctx.result.n_regions


def test_merge_tree_replays_region_counts(P, gpu_ctx):
    name = "rgbd_160x120"
    pts, prm = case_points(P, name), case_params(P, name)
    gpu_ctx.segment(pts, prm)
    a, b, w = gpu_ctx.merge_tree()
    m = gpu_ctx.debug("MERGES").reshape(-1, 3)
    assert np.array_equal(a, m[:, 0]) and np.array_equal(b, m[:, 1]) and w.tobytes() == m[:, 2].tobytes()
    assert len(a) == gpu_ctx.result.n_merges
    S = len(gpu_ctx.debug("SV_LABELS"))
    ts = level_thresholds(w, prm.threshold)
    _, nreg = gpu_ctx.labels_at_thresholds(ts)
    for l, t in enumerate(ts):
        fails = np.nonzero(~(w < t))[0]
        p = int(fails[0]) if len(fails) else len(w)
        assert nreg[l] == S - p                # every merge removes one region


def test_cli_levels_files_equal_separate_runs(tmp_path):
    assert os.path.exists(CLI)
    base = [CLI, "-p", FIXTURE_PCD, "--CVX", "--AL"]
    levels = ["0.1", "0.15", "0.05", "0.2"]
    r = subprocess.run(base + ["-t", "0.2", "--labels", str(tmp_path / "lv"), "--levels", ",".join(levels)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for i, t in enumerate(levels):
        r = subprocess.run(base + ["-t", t, "--labels", str(tmp_path / ("t%d" % i))], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / ("lv.L%d" % i)).read_bytes() == (tmp_path / ("t%d" % i)).read_bytes(), "level %s" % t
    assert (tmp_path / "lv.L3").read_bytes() == (tmp_path / "lv").read_bytes()
