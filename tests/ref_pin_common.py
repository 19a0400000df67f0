"""The reference's OWN merge half and scorer (its clustering, clustering_state, testing and color_utilities sources, compiled unchanged against oracle/ref_shim
into oracle/_ref/libf3ds_ref.so) as a checker, and the cases it is compared on.  Plain numpy + ctypes, no GPU.

tests/test_ref_pin_cpu.py compares it bit for bit with the oracle's restatement on libm (libf3ds_oracle_libm.so) and measures how far the default oracle
(csrc/f3ds_math.h instead of libm) is from it; tests/test_ref_pin_gpu.py compares the HIP merge loop with it.  The library is built where a checkout of the
reference is at hand (oracle/Makefile, REF_DIR) and travels with the tree to a machine that has none.

A case is a supervoxel set + adjacency pairs + parameters.  kind says how far the comparison goes:
  'run'      everything (labels, merge sequence with weight bits, lambda, regions, region adjacency, labelled cloud, scores)
  'tie'      a mass tie or NaN weights: as 'run' against the libm oracle; against the default oracle and the device on labels only, exempt from the same_sequence share
  'throws'   the reference throws; expect = the code the exception maps to (ref_driver.cpp), oracle_expect = what the oracle answers (None: the same)
classes(run) names the classes of REQUIRED a run populates, from the run's own data (which rewrite branches its merges took, whether its weights tie, ...);
the CPU module asserts that no class is empty."""
import collections
import ctypes
import os

import numpy as np

import merge_graphs_common as G
from conftest import ROOT, CpuChecker, _make

REF_DIR = os.environ.get("REF_DIR", "/root/reference")
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libf3ds_ref.so")
LAB, RGB = 0, 1
ND, CVX = 0, 1
MANUAL, ADAPTIVE, EQUALIZATION = 0, 1, 2
PERF = ("voi", "precision", "recall", "fscore", "wov", "fpr", "fnr")
# Largest relative difference between the reference (libm) and the default oracle (csrc/f3ds_math.h) over every case of test_ref_pin_cpu.py whose merge sequence is the
# same, the two frames included: measured on the build machine (glibc 2.35, x86-64; test_distance_to_the_default_oracle prints it), asserted at twice that -- the margin is
# for another libm.  The scorer takes its logarithms from libm on every side (csrc/f3ds_eval.h), so equal labels score equally.  The device equals the default oracle bit
# for bit, so the same bounds hold between the device and the reference (test_ref_pin_gpu.py).
MEASURED = dict(weight=9.28e-05, lambda_=1.08e-07, perf=0.0)
BOUND = {k: 2 * v for k, v in MEASURED.items()}
SAME_SEQUENCE_SHARE = 0.75


def reference_present():
    return os.path.exists(os.path.join(REF_DIR, "src", "clustering.cpp"))


def load_ref():
    """(checker, None) or (None, why not).  Builds the library first where the reference is at hand (a no-op when it is newer than its sources)."""
    if reference_present():
        _make("oracle")
    if not os.path.exists(REF_LIB):
        return None, "oracle/_ref/libf3ds_ref.so is missing" + (" although the reference is at %s: make -C oracle" % REF_DIR if reference_present() else " and there is no reference checkout to build it from")
    chk = CpuChecker(REF_LIB, "f3ds_ref")
    chk.lib.f3ds_ref_lambda.restype = ctypes.c_float
    assert chk.lib.f3ds_ref_uses_libm() == 1, "the reference library is not linked to the libm oracle"
    return chk, None


# ------------------------------------------------------------------------------------------------ calls the shared Handle does not have
def _vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def region_adjacency(chk, h):
    n = ctypes.c_size_t()
    assert chk.fn("region_adjacency")(h.h, None, ctypes.c_size_t(0), ctypes.byref(n)) == 0
    out = np.zeros((n.value, 2), np.uint32)
    assert chk.fn("region_adjacency")(h.h, _vp(out), ctypes.c_size_t(n.value), ctypes.byref(n)) == 0
    return out


def set_truth_points(chk, h, xyz):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    assert chk.fn("set_truth_points")(h.h, _vp(xyz), ctypes.c_size_t(len(xyz))) == 0


def eval_clouds(chk, sxyz, slab, txyz, tlab):
    """Testing(s, t).eval_performance() on two label clouds -> (rc, dict of the seven scores as float32)."""
    sxyz = np.ascontiguousarray(sxyz, np.float32).reshape(-1, 3); txyz = np.ascontiguousarray(txyz, np.float32).reshape(-1, 3)
    slab = np.ascontiguousarray(slab, np.uint32); tlab = np.ascontiguousarray(tlab, np.uint32)
    assert len(slab) == len(sxyz) and len(tlab) == len(txyz)
    out = chk.P.Performance()
    rc = chk.fn("eval_clouds")(_vp(sxyz), _vp(slab), ctypes.c_size_t(len(slab)), _vp(txyz), _vp(tlab), ctypes.c_size_t(len(tlab)), ctypes.byref(out))
    return rc, perf_array(out)


def perf_array(p):
    return np.array([getattr(p, k) for k in PERF], np.float32)


def truth_cloud(oracle, h, truth_point_labels):
    """The labelled voxel cloud main() makes of per-point truth labels (the oracle's: voxelisation is not part of what is pinned here)."""
    t = np.ascontiguousarray(truth_point_labels, np.uint32)
    n = ctypes.c_size_t()
    assert oracle.fn("truth_cloud")(h.h, _vp(t), None, None, ctypes.c_size_t(0), ctypes.byref(n)) in (0, oracle.P.ERR_CAPACITY)
    xyz = np.zeros((n.value, 3), np.float32); lab = np.zeros(n.value, np.uint32)
    assert oracle.fn("truth_cloud")(h.h, _vp(t), _vp(xyz), _vp(lab), ctypes.c_size_t(n.value), ctypes.byref(n)) == 0
    return xyz, lab


def rows(chk, name, a):
    """ciede00 / rgb_eucl of (n, 6) float32 rows -> (n,) float32."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 6)
    out = np.zeros(len(a), np.float32)
    chk.fn(name + "_rows")(_vp(a), ctypes.c_size_t(len(a)), _vp(out))
    return out


def mean_color_rows(chk, rgba, offset):
    rgba = np.ascontiguousarray(rgba, np.uint32); offset = np.ascontiguousarray(offset, np.uint32)
    out = np.zeros((len(offset) - 1, 3), np.float32)
    chk.fn("mean_color_rows")(_vp(rgba), _vp(offset), ctypes.c_size_t(len(offset) - 1), _vp(out))
    return out


# ------------------------------------------------------------------------------------------------ graphs beyond merge_graphs_common's
def _xy_grid(w, h):
    return np.stack([np.tile(np.arange(w), h) * 0.1, np.repeat(np.arange(h), w) * 0.1], axis=1)


def g_scene(seed, w=8, h=8, diagonals=True, n_vox=(4, 9), tilt=0.3):
    """w x h supervoxels of random colours, random unit normals and random tilts of their voxel planes, 4-connected plus diagonals (triangles: merges meet duplicate
    adjacencies and every rewrite branch), centroids off the lattice by a random step so that C = C1 - C2 has three non-zero components."""
    rng = np.random.default_rng(seed)
    S = w * h
    idx = lambda r, c: r * w + c
    edges = [(idx(r, c), idx(r, c + 1)) for r in range(h) for c in range(w - 1)] + [(idx(r, c), idx(r + 1, c)) for r in range(h - 1) for c in range(w)]
    if diagonals:
        edges += [(idx(r, c), idx(r + 1, c + 1)) for r in range(h - 1) for c in range(w - 1)] + [(idx(r, c + 1), idx(r + 1, c)) for r in range(h - 1) for c in range(w - 1)]
    nrm = G._unit(np.concatenate([rng.normal(0, 0.35, (S, 2)), np.ones((S, 1))], axis=1))
    sv, pairs = G._assemble(rng.integers(n_vox[0], n_vox[1] + 1, S), rng.integers(0, 256, (S, 3)), _xy_grid(w, h) + rng.uniform(-0.02, 0.02, (S, 2)), edges, normal=nrm,
                            tilt=rng.uniform(-tilt, tilt, S))
    sv["centroid_xyz"][:, 2] += rng.uniform(-0.03, 0.03, S).astype(np.float32)
    return sv, pairs


def g_pairs_of(sv_pairs, form, extra=()):
    """The same graph with its adjacency listed another way.  'one': kept direction only; 'mixed': every edge in one direction, alternately the kept and the dropped one
    (half the edges vanish in clear_adjacency); extra: rows appended as they are."""
    sv, pairs = sv_pairs
    kept = G.kept_edges(pairs)
    if form == "one":
        out = kept
    elif form == "mixed":
        out = kept.copy(); out[1::2] = out[1::2, ::-1]
    else:
        out = pairs
    if len(extra):
        out = np.vstack([out, np.asarray(extra, np.uint32).reshape(-1, 2)])
    return sv, np.ascontiguousarray(out, np.uint32)


def g_clamp(seed=3):
    """A chain under RGB_EUCL with one black / white edge: delta_c = 441.672943 / 441.672943 = 1, so delta_c * bins == bins and t_c's clamp is what keeps map::at from throwing."""
    rng = np.random.default_rng(seed)
    n = 24
    rgb = rng.integers(0, 256, (n, 3)); rgb[10] = (0, 0, 0); rgb[11] = (255, 255, 255)
    t = rng.uniform(-0.5, 0.5, n)
    return G._assemble(np.full(n, 4), rgb, G._chain_xy(n), G._chain_edges(n), normal=G._unit(np.stack([np.zeros(n), np.sin(t), np.cos(t)], axis=1)))


def g_delta_g_one(seed=4):
    """... and one edge with delta_g = (0 + 3 + 0) / 3 = 1 exactly (normals (3, 0, 0) and (0, 0, 0) along the chain's axis): t_g has no clamp."""
    sv, pairs = g_clamp(seed)
    sv["normal"][4] = (3, 0, 0); sv["normal"][5] = (0, 0, 0)
    sv["normal"][3] = (0, 0, 0)       # (the edge on the other side of (3, 0, 0) is 1 as well; no delta_g exceeds 1: compute_cdf indexes its bins with it)
    return sv, pairs


def g_cheapest_first():
    """g_scene(47, 6, 6) with supervoxels 1 and 2 one colour step apart: under MANUAL_LAMBDA with lambda = 1 (the colours alone decide) their adjacency is merged first."""
    sv, pairs = g_scene(47, 6, 6)
    a, b = int(sv["voxel_offset"][0]), int(sv["voxel_offset"][1]); c = int(sv["voxel_offset"][2])
    sv["voxel_rgba"][a:b] = (100 << 16) | (110 << 8) | 120
    sv["voxel_rgba"][b:c] = (100 << 16) | (111 << 8) | 120
    return sv, pairs


def g_single():
    return G._assemble([5], [(10, 200, 30)], [(0.0, 0.0)], [])


def g_no_edges(seed=5):
    rng = np.random.default_rng(seed)
    return G._assemble(np.full(6, 4), rng.integers(0, 256, (6, 3)), G._chain_xy(6), [])


def g_all_same(n=12):
    """One colour AND one normal: delta_c = delta_g = 0 everywhere, lambda = 0 / 0."""
    return G._assemble(np.full(n, 4), np.tile(np.array([90, 120, 60]), (n, 1)), G._chain_xy(n), G._chain_edges(n))


# ------------------------------------------------------------------------------------------------ the cases
RCase = collections.namedtuple("RCase", "name build prm kind expect oracle_expect")
CASES = []


def rcase(name, build, kind="run", expect=0, oracle_expect=None, **prm):
    CASES.append(RCase(name, build, dict(prm), kind, expect, oracle_expect))


CM = {LAB: "lab", RGB: "rgb"}; GM = {ND: "nd", CVX: "cvx"}; MG = {MANUAL: "manual", ADAPTIVE: "adaptive", EQUALIZATION: "eq"}
T_OF = {MANUAL: 0.14, ADAPTIVE: 0.14, EQUALIZATION: 0.45}      # (RGB_EUCL distances of random colours are larger: + 0.1)
for _c in (LAB, RGB):
    for _g in (ND, CVX):
        for _m in (MANUAL, ADAPTIVE, EQUALIZATION):
            rcase("scene8x8-%s-%s-%s" % (CM[_c], GM[_g], MG[_m]), lambda s=11 + 3 * _c + 5 * _g + 7 * _m: g_scene(s), color_metric=_c, geom_metric=_g, merging=_m,
                  threshold=T_OF[_m] + (0.1 if _c == RGB and _m != EQUALIZATION else 0.0))
for _l in (0.0, 0.5, 1.0):
    rcase("scene6x6-lambda-%g" % _l, lambda: g_scene(41, 6, 6), merging=MANUAL, **{"lambda": _l, "threshold": 0.1 if _l == 1.0 else 0.17})
for _b in (500, 4, 1, 0):
    rcase("scene6x6-bins-%d" % _b, lambda: g_scene(43, 6, 6), merging=EQUALIZATION, bins=_b, threshold=0.6 if _b != 1 else 1.5)
rcase("clamp-eq-rgb", g_clamp, color_metric=RGB, merging=EQUALIZATION, bins=500, threshold=0.4)
rcase("clamp-eq-rgb-bins7", g_clamp, color_metric=RGB, merging=EQUALIZATION, bins=7, threshold=0.4)
rcase("delta-g-one-eq", g_delta_g_one, kind="throws", expect=-9, color_metric=RGB, merging=EQUALIZATION, bins=500, threshold=0.4)
rcase("delta-g-one-adaptive", g_delta_g_one, color_metric=RGB, merging=ADAPTIVE, threshold=0.2)      # (the same graph where nothing throws)
# adaptive-lambda degenerates
rcase("grid8-flat-adaptive", lambda: G.make_graph("grid", 0, w=8, h=8), kind="tie", merging=ADAPTIVE, threshold=0.2)                   # lambda = 0: every weight 0
rcase("chain-all-same-adaptive", g_all_same, kind="tie", merging=ADAPTIVE, threshold=0.2)                                             # lambda = NaN: no merge
rcase("grid8-all-equal-manual", lambda: G.make_graph("grid", 0, w=8, h=8, colours="equal"), kind="tie", merging=MANUAL, threshold=0.2)
rcase("single", g_single, merging=ADAPTIVE, threshold=0.2)
rcase("no-edges", g_no_edges, merging=ADAPTIVE, threshold=0.2)
# adjacency input forms
rcase("scene6x6-one-direction", lambda: g_pairs_of(g_scene(47, 6, 6), "one"), merging=ADAPTIVE, threshold=0.22)
rcase("scene6x6-mixed-directions", lambda: g_pairs_of(g_scene(47, 6, 6), "mixed"), merging=ADAPTIVE, threshold=0.22)
rcase("scene6x6-both-directions", lambda: g_scene(47, 6, 6), merging=ADAPTIVE, threshold=0.22)
rcase("scene6x6-missing-label", lambda: g_pairs_of(g_scene(47, 6, 6), "both", [(3, 900)]), kind="throws", expect=-13, merging=ADAPTIVE, threshold=0.15)
rcase("scene6x6-missing-label-eq", lambda: g_pairs_of(g_scene(47, 6, 6), "both", [(3, 900)]), kind="throws", expect=-13, merging=EQUALIZATION, threshold=0.15)
rcase("scene6x6-missing-label-dropped", lambda: g_pairs_of(g_scene(47, 6, 6), "both", [(900, 3)]), merging=ADAPTIVE, threshold=0.15)
# (a pair listed twice and a self-pair: the oracle and the device refuse them up front with ERR_ARG, include/f3ds.h; what the reference does is in test_ref_pin_cpu.py)
rcase("scene6x6-pair-twice", lambda: g_pairs_of(g_cheapest_first(), "both", [(1, 2)]), kind="throws", expect=-13, oracle_expect=-1, merging=MANUAL, **{"lambda": 1.0, "threshold": 0.1})
rcase("scene6x6-pair-twice-never-merged", lambda: g_pairs_of(g_cheapest_first(), "both", [(1, 2)]), kind="throws", expect=0, oracle_expect=-1, merging=MANUAL, **{"lambda": 1.0, "threshold": 0.0})
rcase("scene6x6-self-pair", lambda: g_pairs_of(g_scene(47, 6, 6), "both", [(4, 4)]), kind="throws", expect=None, oracle_expect=-1, merging=MANUAL, threshold=0.1)
# thresholds and the rewrite branches
rcase("scene10x10-to-the-end", lambda: g_scene(53, 10, 10), merging=MANUAL, threshold=5.0)
rcase("scene6x6-threshold-0", lambda: g_scene(47, 6, 6), merging=ADAPTIVE, threshold=0.0)
for _n in ("clique12-manual", "clique12-adaptive", "clique12-equalization", "clique40-adaptive", "tie3-group-min-manual", "tie3-group-second-adaptive", "tie3-lanes-min-manual", "tie2-group-min-equalization",
           "grid12-tie3", "grid12-tie3-second", "big-many-leaves", "monotone-chain-manual", "ladder20-manual", "ladder20-adaptive", "chains8x40-equalization", "chain-E257"):
    _c = G.CASE[_n]
    rcase("mg-" + _n, lambda n=_n: G.graph_of(n), merging=_c.merging, threshold=_c.threshold)
rcase("star200", lambda: G.make_graph("star", 2, spokes=200, close=30, hub_vox=100, tilt=0.2), merging=MANUAL, threshold=0.01)

CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)
LARGEST = "mg-chains8x40-equalization"        # 320 supervoxels: the case the GPU module also runs in the other merge-kernel layouts

REQUIRED = (["combo %s %s %s" % (CM[c], GM[g], MG[m]) for c in CM for g in GM for m in MG] + ["manual lambda 0", "manual lambda 0.5", "manual lambda 1"] +
            ["eq bins 500", "eq bins 4", "eq bins 1", "eq bins 0", "eq clamp delta_c * bins == bins", "eq delta_g == 1 throws"] +
            ["adaptive lambda 0 mass tie", "adaptive lambda NaN no merge", "one supervoxel", "no edges"] +
            ["pairs in both directions", "pairs in one direction", "pair listed twice", "self pair", "missing label", "missing label in a dropped pair"] +
            ["branch: touches first", "branch: first == second", "branch: second == second, first below", "branch: second == second, first above", "branch: duplicate dropped",
             "equal weights at the head", "threshold 0", "threshold above every weight", "merged to one region"])




# ------------------------------------------------------------------------------------------------ runs
_graphs = {}


def graph(name):
    if name not in _graphs:
        _graphs[name] = CASE[name].build()
    return _graphs[name]


def params(P, c):
    return P.default_params(**c.prm)


def truth_of(sv):
    """Per-voxel truth labels of a synthetic graph: five blocks of supervoxels, every seventh voxel moved to the next block (impure segments, ids that skip values)."""
    S = len(sv["label"])
    owner = np.repeat(np.arange(S), np.diff(sv["voxel_offset"]).astype(np.int64))
    t = (owner * 5) // max(S, 1) * 3
    t[::7] += 3
    return t.astype(np.uint32)


def region_adjacency_of(h):
    """weight2adj(state.weight_map) from the oracle's arrays: every initial edge between the labels its endpoints ended in, deduplicated, sorted."""
    labels = h.get("SV_LABELS"); root = h.get("SV_REGION"); e = h.get("EDGES").reshape(-1, 2)
    lut = dict(zip(labels.tolist(), root.tolist()))
    out = set()
    for a, b in e:
        p, q = lut[int(a)], lut[int(b)]
        if p != q:
            out.add((min(p, q), max(p, q)))
    return np.array(sorted(out), np.uint32).reshape(-1, 2)


def sorted_rows(a):
    a = np.asarray(a, np.uint32).reshape(-1, 2)
    return a[np.lexsort((a[:, 1], a[:, 0]))]


Run = collections.namedtuple("Run", "rc region vlab res h merges lam regions radj cloud perf")


def run(chk, sv, pairs, prm, is_ref):
    """One cluster_supervoxels call and everything that is compared of it.  perf: the seven scores of its labelled cloud against truth_of(sv)."""
    rc, region, vlab, res, h = chk.cluster_supervoxels(sv, pairs, prm)
    if rc:
        return Run(rc, None, None, None, None, None, None, None, None, None, None)
    cloud = h.voxel_cloud()
    prc, perf = eval_clouds(chk, cloud[0], cloud[1], sv["voxel_xyz"], truth_of(sv))
    assert prc == 0
    radj = sorted_rows(region_adjacency(chk, h)) if is_ref else region_adjacency_of(h)
    return Run(0, region, vlab, res, h, h.get("MERGES").reshape(-1, 3), np.float32(res.lambda_), h.regions(), radj, cloud, perf)


_runs = {}


def case_run(which, chk, P, name):
    """The run of a case by one checker ('ref' | 'libm' | 'math'), made once per process and shared read-only."""
    key = (which, name)
    if key not in _runs:
        sv, pairs = graph(name)
        _runs[key] = run(chk, sv, pairs, params(P, CASE[name]), which == "ref")
    return _runs[key]


def same_sequence(a, b):
    return a.rc == 0 and b.rc == 0 and np.array_equal(a.merges[:, :2], b.merges[:, :2])


def rel_diff(a, b):
    """Largest |a - b| / max(|a|, |b|) over the entries that differ (0 where all are equal; NaN equals NaN)."""
    a = np.asarray(a, np.float64).reshape(-1); b = np.asarray(b, np.float64).reshape(-1)
    both_nan = np.isnan(a) & np.isnan(b)
    d = np.abs(a - b); m = np.maximum(np.abs(a), np.abs(b))
    ok = ~both_nan & (d > 0)
    return float((d[ok] / m[ok]).max()) if ok.any() else 0.0


# ------------------------------------------------------------------------------------------------ which classes a run populates
def merge_branches(kept, merges):
    """Which branch of merge()'s rewrite loop (src/clustering.cpp:436-467) every adjacency took, per merge of the log; a structural replay on label pairs (the order
    of the map does not matter for the counts)."""
    cur = set(map(tuple, np.asarray(kept).reshape(-1, 2).tolist()))
    n = collections.Counter()
    for a, b in np.asarray(merges).reshape(-1, 3)[:, :2].tolist():
        assert (a, b) in cur
        new = set()
        for p, q in cur:
            if (p, q) == (a, b):
                continue
            if p == a or q == a:
                br, e = "branch: touches first", (p, q)
            elif p == b:
                br, e = "branch: first == second", (a, q)
            elif q == b:
                br, e = ("branch: second == second, first below", (p, a)) if p < a else ("branch: second == second, first above", (a, p))
            else:
                new.add((p, q))
                continue
            n[br] += 1
            if e in new:
                n["branch: duplicate dropped"] += 1
            new.add(e)
        cur = new
    return n


def classes(c, sv, pairs, prm, o, twin_delta_g_max=None):
    """The classes of REQUIRED that case c populates.  o: the libm oracle's Run of it (rc != 0 for a case that throws)."""
    out = set()
    S = len(sv["label"]); kept = G.kept_edges(pairs)
    rows_ = set(map(tuple, pairs.tolist()))
    if c.kind == "throws":
        if c.expect == -9 and twin_delta_g_max == 1.0:
            out.add("eq delta_g == 1 throws")
        if len(pairs) != len(rows_) and c.expect == -13:
            out.add("pair listed twice")
        if any(a == b for a, b in rows_):
            out.add("self pair")
        if any(a <= b and (a > S or b > S) for a, b in rows_) and c.expect == -13:
            out.add("missing label")
        return out
    M = len(o.merges); w = o.h.get("EDGE_WEIGHTS"); d = o.h.get("EDGE_DELTAS").reshape(-1, 2)
    many = M >= 5 and o.res.n_regions > 1
    if many and c.kind == "run":
        out.add("combo %s %s %s" % (CM[prm.color_metric], GM[prm.geom_metric], MG[prm.merging]))
        if prm.merging == MANUAL and "lambda" in c.prm:
            out.add("manual lambda %g" % c.prm["lambda"])
        if prm.merging == EQUALIZATION and "bins" in c.prm and "scene" in c.name:
            out.add("eq bins %d" % c.prm["bins"])
    if M >= 5 and prm.merging == EQUALIZATION and "bins" in c.prm and c.prm["bins"] == 1:
        out.add("eq bins 1")                                              # (one bin: every weight is 1, everything merges below 1.5)
    if prm.merging == EQUALIZATION and len(d) and (np.floor(d[:, 0] * np.float32(prm.bins or 500)) == (prm.bins or 500)).any():
        out.add("eq clamp delta_c * bins == bins")
    if prm.merging == ADAPTIVE and o.lam == 0 and len(w) and (w == 0).all() and M >= 10:
        out.add("adaptive lambda 0 mass tie")
    if prm.merging == ADAPTIVE and np.isnan(o.lam) and M == 0 and len(w):
        out.add("adaptive lambda NaN no merge")
    if S == 1:
        out.add("one supervoxel")
    if S > 1 and len(pairs) == 0:
        out.add("no edges")
    if many and len(kept) and all((b, a) in rows_ for a, b in kept.tolist()):
        out.add("pairs in both directions")
    if many and len(kept) and not any((b, a) in rows_ for a, b in kept.tolist()):
        out.add("pairs in one direction")
    if any(a > b and a > S for a, b in rows_):
        out.add("missing label in a dropped pair")
    out |= set(k for k, v in merge_branches(o.h.get("EDGES").reshape(-1, 2), o.merges).items() if v)
    if len(w) and np.isfinite(w).all() and len(np.unique(w)) > 2 and int((w == w.min()).sum()) >= 2 and w.min() < prm.threshold:
        out.add("equal weights at the head")
    if prm.threshold == 0 and M == 0 and len(w):
        out.add("threshold 0")
    if M and len(o.radj) == 0 and prm.threshold > o.merges[:, 2].view(np.float32).max():
        out.add("threshold above every weight")
    if M and o.res.n_regions == 1:
        out.add("merged to one region")
    return out
