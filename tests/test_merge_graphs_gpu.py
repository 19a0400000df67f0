"""The HIP merge loop (d_merge_il_t<4 | 8 waves, keys in LDS | global memory>, with and without the speculative second merge, and the all-global d_merge) on the synthetic
supervoxel graphs of merge_graphs_common.py, against the oracle's cluster_supervoxels bit for bit: ties of the minimum key, the uniqueness test of the runner-up, every
stand-down of the speculation, the touched list over its cap and the tie path's own fallback, the event regrow, staging chunks, duplicate adjacencies, NaN keys and the size
edges of the LDS layouts.  tests/test_merge_graphs_cpu.py shows that the oracle's run of each case meets the condition that makes it exercise its path.

The oracle runs are shared with the CPU module's (one per case and process; seconds per case in that module's docstring); a case's kernel time is milliseconds."""
import json
import os

import numpy as np
import pytest

import merge_graphs_common as G
from conftest import ROOT, first_mismatch, sha_of
from golden_cases import case_params, case_points
from test_cluster_supervoxels import check_against, map_labels, relabel
from test_gpu_parity import MERGE_VARIANTS

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in G.CASES]
VARIANT_NAMES = [c.name for c in G.CASES if c.variants]
CONTINUED = [c.name for c in G.CASES if c.cont]
RERUN_GLOBAL = "runs again with the global-memory kernel"
RERUN_ROOM = "runs again with more history / leaf-pool room"


@pytest.fixture(scope="module")
def ctx(P):
    if P.device_count() < 1:
        pytest.fail("GPU test selected but libf3ds sees no HIP device (no CPU fallback exists)")
    c = P.Context(0)
    yield c
    c.close()


def variant_id(v):
    return "-".join("%s" % x for x in v.values()) or "default"


def expected_layout(P, case, env, n_edges):
    """What Context.merge_layout() has to say after `case` ran under the switches `env`."""
    if "F3DS_FORCE_GLOBAL_MERGE" in env or case.layout == "fallback":
        return (0, 0)
    if "F3DS_MERGE_NW" in env:
        nw, res = int(env["F3DS_MERGE_NW"]), 2 if env["F3DS_MERGE_KEYS"] == "lds" else 0
        assert P.merge_layout_info(n_edges, nw, res)[3], "case %s does not fit the layout it is forced into" % case.name
        return (nw, res)
    return (8, 0) if case.layout == "global_keys" else (8, 2)


def run_case(P, oracle, context, name, env, monkeypatch, capfd):
    """One case under one set of switches: every merge-side array, the counts, lambda and both returned arrays against the oracle; the layout that ran; and, on stderr,
    whether the stage ran again (F3DS_TRACE_ERR is read per call)."""
    r = G.oracle_run(oracle, P, name)
    with monkeypatch.context() as mp:
        mp.setenv("F3DS_TRACE_ERR", "1")
        for k, v in env.items():
            mp.setenv(k, v)
        capfd.readouterr()
        region, vlab = context.cluster_supervoxels(r.sv, r.pairs, G.params_of(P, r.case))
        err = capfd.readouterr().err
    where = "%s under %s" % (name, variant_id(env))
    want = expected_layout(P, r.case, env, len(r.edges))
    assert context.merge_layout() == want, where
    assert (RERUN_GLOBAL in err) == (r.case.layout == "fallback" and "F3DS_FORCE_GLOBAL_MERGE" not in env), (where, err)
    if r.case.cond[0] != "events":
        assert RERUN_ROOM not in err, (where, err)
    try:
        check_against(context, r.h, region, vlab, r.sv, P, r.res, r.region, r.vlab)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (where, e)) from e
    return r, err


@pytest.mark.parametrize("name", NAMES)
def test_merge_graph_in_the_default_layout(P, oracle, ctx, monkeypatch, capfd, name):
    """Every case as a lone call gets it: 8 waves, keys in LDS while they fit.  Cases that name further switch settings (the 4-wave layouts at their own size edges) run under those too."""
    case = G.CASE[name]
    fresh = P.Context(0) if case.cond[0] == "events" else None      # (the event room a context has grown to stays: the regrow needs a context that has not seen it)
    try:
        for env in ({},) + case.envs:
            r, err = run_case(P, oracle, fresh or ctx, name, env, monkeypatch, capfd)
            if case.cond[0] == "events" and not env:
                assert RERUN_ROOM in err, err
        kept = G.kept_edges(r.pairs)
        assert np.array_equal((fresh or ctx).supervoxel_adjacency(), kept)
    finally:
        if fresh:
            fresh.close()


@pytest.mark.parametrize("name", VARIANT_NAMES)
def test_merge_graph_in_every_merge_kernel_layout(P, oracle, ctx, monkeypatch, capfd, name):
    """Families 1-7 and 9 in all nine variants: 4 or 8 waves x keys in LDS or global memory x speculation on or off, and d_merge forced.  A case that has to fall back
    (touched list or tie list over MC_TL_CAP) ends in d_merge from every LDS layout."""
    case = G.CASE[name]
    assert len(MERGE_VARIANTS) == 9
    for env in MERGE_VARIANTS:
        context = P.Context(0) if case.cond[0] == "events" else ctx
        try:
            r, err = run_case(P, oracle, context, name, env, monkeypatch, capfd)
            if case.cond[0] == "events":
                assert RERUN_ROOM in err, (variant_id(env), err)
        finally:
            if context is not ctx:
                context.close()


@pytest.mark.parametrize("name", G.RELABELLED)
def test_merge_graph_under_sparse_keys_and_permuted_rows(P, oracle, ctx, name):
    """Every family once more with 32-bit keys far apart and the rows in another order: the same merge weights, endpoints mapped through the key table."""
    r = G.oracle_run(oracle, P, name)
    sv2, pairs2, lut, perm, vox = relabel(r.sv, r.pairs, np.random.default_rng(21))
    prm = G.params_of(P, r.case)
    context = P.Context(0) if r.case.cond[0] == "events" else ctx
    try:
        region, vlab = context.cluster_supervoxels(sv2, pairs2, prm)
        rc, oregion, ovlab, ores, h2 = oracle.cluster_supervoxels(sv2, pairs2, prm)
        assert rc == 0
        check_against(context, h2, region, vlab, sv2, P, ores, oregion, ovlab)
        m2 = context.debug("MERGES").reshape(-1, 3)
        assert np.array_equal(m2[:, 2], r.merges[:, 2]) and np.array_equal(m2[:, :2], map_labels(r.merges[:, :2], lut))
        assert np.array_equal(vlab, r.vlab[vox])
    finally:
        if context is not ctx:
            context.close()


def labels_of(h, n):
    """Region id per input voxel from an oracle handle (get_labeled_cloud's ids through the voxel index of region_voxels)."""
    xyz, rgba, idx = h.region_voxels(); _, lab, _ = h.voxel_cloud()
    out = np.zeros(n, np.uint32); out[idx] = lab
    return out


@pytest.mark.parametrize("name", CONTINUED)
def test_recluster_and_levels_continue_on_the_state_of_a_merge_graph(P, oracle, monkeypatch, name):
    """After the mass ties, the event regrow and the big absorbed regions: f3ds_recluster at lower thresholds equals the oracle handle's cluster(), f3ds_labels_at_thresholds
    equals recluster at each of its thresholds -- one of them exactly a logged weight (a t_l equal to a logged weight stops at that merge) --, and the context then segments
    a frame as if nothing had been (golden labels)."""
    r = G.oracle_run(oracle, P, name)
    prm = G.params_of(P, r.case)
    context = P.Context(0)
    region, vlab = context.cluster_supervoxels(r.sv, r.pairs, prm)
    rc, oregion, ovlab, ores, h = oracle.cluster_supervoxels(r.sv, r.pairs, prm)       # (a handle of its own: cluster() below changes it, the shared run stays as it is)
    assert rc == 0 and np.array_equal(vlab, ovlab) and np.array_equal(region, oregion)
    w = r.merges[:, 2].view(np.float32)
    T = np.float32(r.case.threshold)
    logged = w[len(w) // 2]
    # the three smallest of: logged weights an eighth, a quarter and half way through the log (cheap for the oracle), T / 2, T
    ts = np.array(sorted({float(w[len(w) // 8]), float(w[len(w) // 4]), float(logged), float(T * np.float32(0.5)), float(T)})[:3], np.float32)
    assert len(ts) == 3 and (ts <= T).all() and np.isin(ts, w).any()
    levels, nreg = context.labels_at_thresholds(ts)
    for l, t in enumerate(ts):
        p2 = prm.copy(); p2.threshold = float(t)
        got = context.recluster(p2)
        rc, _, ores2 = h.cluster(p2, 0)
        assert rc == 0 and (context.result.n_merges, context.result.n_regions) == (ores2.n_merges, ores2.n_regions), (name, t)
        stop = np.nonzero(~(w < t))[0]                                                 # the run at t is the run at T up to its first merge that is not below t
        assert ores2.n_merges == (int(stop[0]) if len(stop) else len(w)), (name, t)
        assert first_mismatch("MERGES", context.debug("MERGES"), h.get("MERGES")) is None
        assert np.array_equal(got, labels_of(h, len(vlab))), (name, t)
        assert np.array_equal(levels[l], got) and nreg[l] == ores2.n_regions, (name, t)
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_golden.json")))
    lab = context.segment(case_points(P, "rgbd_160x120"), case_params(P, "rgbd_160x120"))
    assert sha_of(lab) == gold["rgbd_160x120"]["labels_sha256"]
    assert sha_of(context.debug("MERGES")) == gold["rgbd_160x120"]["sha256"]["MERGES"]
    context.close()
