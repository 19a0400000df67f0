"""Batch calls whose frames disagree on every decision the host takes for the whole batch (segment_batch_from, run_cluster and flush in csrc/f3ds_hip.hip): the launch
width and LDS of every dispatch, the key widths of the sorts, whether the point sort moves (key, index) pairs, whether stage 0 takes the tile path, what a context
remembers of a refusal, frames that leave the batch, the adjacency pass and the merge stage that run again for all frames because one frame needed it, the merge layout,
the normals kernel.

Plain numpy, no GPU.  MIXES lists every batch: its frames (lattice clouds of vccs_clouds_common.py at voxel_res = R), one set of parameters, the environment of the call,
the condition that makes it the mix it is named for, and what the call has to show.  A condition is checked from the oracle's lone runs of the frames and from the constants
restated below (HOST_CONSTANTS: test_batch_mix_cpu.py compares each with the library's own, P.constant(name)), never from the code under test: tests/test_batch_mix_cpu.py asserts every condition and that the
emulation equals the oracle on every frame, tests/test_batch_mix_gpu.py runs every mix through segment_batch and compares every frame with its lone oracle run.

The reference of a frame is oracle.segment(frame, prm) on that frame alone.  Its arrays are copied when the run is made (Snapshot): a later cluster() on the oracle's
handle, which the tests of the contexts' state need, leaves them as they were."""
import collections

import numpy as np

import vccs_clouds_common as C
from conftest import ALL_DEBUG
from merge_graphs_common import FIT_EDGES
from vccs_clouds_common import R, _count_frame, _one_dense, _with_far, block, census, cloud

# ---- the constants of the host logic the mixes are sized by (checked against the library's own by test_batch_mix_cpu.py)
VT_CNT_BITS = 14            # bits of a tile descriptor's key that hold the entry's point count
VT_TILE = 4096              # points per tile of stage 0's tile path
N_BLOCK_DEPTH_MAX = 12      # deepest grid whose neighbour search goes through the 4x4x4 block table
DENSE_PENALTY = 8           # calls a context stays off the tile path after its first refusal ...
DENSE_PENALTY_CAP = 1024    # ... doubled at every further refusal, up to this
EDGE_MULT = 32              # adjacency list room per seed: S0 * edge_mult + EDGE_EXTRA ...
EDGE_EXTRA = 1024
EDGE_GROW = 4               # ... times this at every overflow
NORMALS_256_FRAMES = 16     # d_normals_t<256> replaces <384> in calls of this many frames
GRID_TARGET = 3072          # workgroups of a streaming kernel for all frames of a call together
WIDE_CAP = 2048             # ... of a gathering kernel, per frame
TILE_MIN_FRAMES = 4         # a call of fewer contexts takes the sort path
KEY_BITS = 64               # a sort key is one 64-bit word
ILIST_SHORT_EXTRA = 16      # entries of the incident-list pool of a frame without adjacencies under F3DS_ILIST_SLACK < 32 (2 E + slack * E * mult + 16)

HOST_CONSTANTS = {       # name of P.constant() -> the value the mixes assume
    "VT_CNT_BITS": VT_CNT_BITS, "VT_TILE": VT_TILE, "N_BLOCK_DEPTH_MAX": N_BLOCK_DEPTH_MAX, "DENSE_PENALTY": DENSE_PENALTY, "DENSE_PENALTY_STEP": 2,
    "DENSE_PENALTY_CAP": DENSE_PENALTY_CAP, "EDGE_MULT": EDGE_MULT, "EDGE_EXTRA": EDGE_EXTRA, "GROW": EDGE_GROW, "EDGE_MULT_CAP": 1 << 14, "EV_MULT_CAP": 16384,
    "POOL_MULT_CAP": 64, "ILIST_MULT_CAP": 4096, "NORMALS_256_FRAMES": NORMALS_256_FRAMES, "GRID_TARGET": GRID_TARGET, "GRID_MIN": 8, "WIDE_CAP": WIDE_CAP,
    "TILE_MIN_CONTEXTS": TILE_MIN_FRAMES, "ILIST_SLACK": 32, "ILIST_EXTRA_SHORT": ILIST_SHORT_EXTRA, "ILIST_EXTRA": 1024, "KEY_BITS": KEY_BITS,
    "OVF_EDGE_LIST": 3, "OVF_DENSE_VOXEL": 6, "OVF_TILE_VOXELS": 7,      # the reasons the F3DS_TRACE_ERR lines of the reruns carry
}
# the grid P.stage0_plan is compared with predict_stage0 on (test_batch_mix_cpu.py)
PLAN_DEPTHS = tuple(range(1, 22))
PLAN_POINTS = (1, 2, 515, 4095, 4096, 4097, 4618, 1 << 20)
PLAN_CONTEXTS = (1, 3, 4, 16)
PLAN_VOX_TILES = (None, "0", "2")      # F3DS_VOX_TILES: unset, the sort path, the tile path for calls of any size


# ------------------------------------------------------------------------------------------------ the two formulas of segment_batch_from
def bits_for(x):
    """Bits the values 0..x need (bits_for of the host code)."""
    return int(x).bit_length()


def tile_key_bits(depths, n_points):
    """Key bits the tile path needs for a batch of live frames: 3 maxd + tile_bits + VT_CNT_BITS."""
    tiles = max(1, max((n + VT_TILE - 1) // VT_TILE for n in n_points))
    return 3 * max(depths) + bits_for(tiles - 1) + VT_CNT_BITS


def sort_key_bits(depths, n_points):
    """Key bits of the one-word point sort: 3 maxd + 1 + idxbits."""
    return 3 * max(depths) + 1 + bits_for(max(1, max(n_points)) - 1)


def predict_stage0(depths, n_points, n_contexts, vox_tiles, sort_pairs=False):
    """(stage0_path() of every live frame, form of the point sort or None) for a batch whose live frames have these octree depths and point counts; vox_tiles: the value
    of F3DS_VOX_TILES (None: unset; "2": the tile path for calls of fewer than four contexts too); sort_pairs: F3DS_SORT_PAIRS, which implies the sort path.  No frame of
    the batch may be one the tile path refuses after it ran (a dense voxel, a tile of too many voxels)."""
    wanted = vox_tiles != "0" and not sort_pairs and (n_contexts >= TILE_MIN_FRAMES or vox_tiles == "2")
    if wanted and tile_key_bits(depths, n_points) <= KEY_BITS:
        return "tiles", None
    return "sort", "pairs" if sort_pairs or sort_key_bits(depths, n_points) > KEY_BITS else "one-word"


def predict_batch_path(runs, n_contexts, vox_tiles=None):
    """stage0_path() of every live frame of a batch, from the oracle's runs: the formulas above on the live frames (dead ones have left by then; the contexts of the
    call count all the same), and "sort" for all when the census of one frame says the tile path refuses it after it ran (predicted_stage0 of vccs_clouds_common.py:
    a voxel of more than VL_MAX_RUN points, a tile of more than VT_ENT_MAX voxels).  For fresh contexts."""
    live = [r for r in runs if r.res.n_voxels]
    if not live:
        return None
    path, _ = predict_stage0([int(r.res.octree_depth) for r in live], [len(r.pts) for r in live], n_contexts, vox_tiles)
    if path == "tiles" and any(C.predicted_stage0(r.census, int(r.res.octree_depth)) == "sort" for r in live):
        path = "sort"
    return path


# ------------------------------------------------------------------------------------------------ the frames
FAR_OF_DEPTH = {13: 5000, 16: 35000, 17: 70000, 18: 140000, 19: 300000, 20: 600000, 21: 1100000}      # block(8, 8, 8) and one voxel this many cells away: the octree depth


def _all_nan():
    pts = cloud(block(8, 8, 8), R).copy()
    pts[:, :3] = np.nan
    return pts


FRAMES = {
    "one-point": lambda: cloud([[0, 0, 0]], R, anchor=False),
    "block3x1x1": lambda: cloud(block(3, 1, 1), R),
    "block8": lambda: cloud(block(8, 8, 8), R),
    "far17-wide": lambda: cloud(_with_far(block(8, 8, 8), [(FAR_OF_DEPTH[17], 3000, 100)]), R, per_cell=9),      # 4 619 points: two tiles, 13 index bits
    "count4097": lambda: _count_frame(4097),
    "block12-random": lambda: cloud(block(12, 12, 12), R, rgba="random"),
    "block14-random": lambda: cloud(block(14, 14, 14), R, rgba="random"),
    "block24-random": lambda: cloud(block(24, 24, 24), R, rgba="random"),
    "plane64-grey": lambda: cloud(block(64, 64, 1), R),
    "empty": lambda: np.zeros((0, 4), np.float32),
    "all-nan": _all_nan,
    "one-dense-257": lambda: _one_dense(257),
    "s-ordered": lambda: C.frame_of("s-ordered").copy(),
}
for _d, _f in FAR_OF_DEPTH.items():
    FRAMES["far%d" % _d] = (lambda f: lambda: cloud(_with_far(block(8, 8, 8), [(f, 3000, 100)]), R))(_f)
DEPTH_OF = dict({"one-point": 1, "block3x1x1": 2, "block8": 3, "far17-wide": 17}, **{"far%d" % d: d for d in FAR_OF_DEPTH})

_frames = {}


def frame_of(name):
    if name not in _frames:
        pts = np.ascontiguousarray(FRAMES[name](), np.float32)
        pts.setflags(write=False)
        _frames[name] = pts
    return _frames[name]


# ------------------------------------------------------------------------------------------------ the parameter sets
DEFAULT = dict(voxel_res=R, seed_res=5 * R, use_transform=0)
SEED_R = dict(voxel_res=R, seed_res=R, use_transform=0)                                                           # every voxel a seed
MANUAL_2R = dict(voxel_res=R, seed_res=2 * R, use_transform=0, merging=0, lambda_=0.5, threshold=1.0)         # manual lambda 0.5: hundreds of merges on random colours
# what recluster() is asked after a batch: another threshold, another geometric metric, another merging mode than either set above
RECLUSTER = dict(geom_metric=0, color_metric=1, merging=0, lambda_=0.3, threshold=0.4)


PARAMS = {"default": DEFAULT, "seed-r": SEED_R, "manual-2r": MANUAL_2R}


def params_of(P, params, **over):
    """The f3ds_params of a parameter set (by its name in PARAMS), with overrides."""
    kw = dict(PARAMS[params]); kw.update(over)
    assert P.MANUAL_LAMBDA == 0 and P.NORMALS_DIFF == 0 and P.RGB_EUCL == 1
    return P.launch_params(**kw)


# ------------------------------------------------------------------------------------------------ the oracle's runs
class Snapshot:
    """The oracle's arrays of one run, copied when it was made (get() as a handle's)."""

    def __init__(self, handle):
        self.arrays = {}
        for w in ALL_DEBUG + ["VOXEL_NEIGHBORS"]:
            a = handle.get(w).copy(); a.setflags(write=False)
            self.arrays[w] = a

    def get(self, name):
        return self.arrays[name]


Run = collections.namedtuple("Run", "frame pts prm labels res h census seconds live reclustered")
_runs = {}


def _key(params):
    return tuple(sorted(params.items()))


def oracle_run(oracle, P, frame, params):
    """The oracle's lone run of a frame under a parameter set, made once per process and shared by every test that needs it.  h: the arrays as they were after the
    run; live: the oracle's handle (for cluster()); census: None for a frame without voxels."""
    key = (frame, params)
    if key not in _runs:
        import time
        pts, prm = frame_of(frame), params_of(P, params)
        t0 = time.perf_counter()
        rc, labels, res, h = oracle.segment(pts, prm)
        dt = time.perf_counter() - t0
        assert rc == 0, "the oracle refuses frame %s: %d" % (frame, rc)
        labels.setflags(write=False)
        snap = Snapshot(h)
        _runs[key] = Run(frame, pts, prm, labels, res, snap, census(P, snap, res) if res.n_voxels else None, dt, h, {})
    return _runs[key]


def oracle_recluster(P, run, params, over=RECLUSTER):
    """(labels, n_merges, n_regions, n_supervoxels) of cluster() with other clustering parameters on the oracle's handle of a run, made once."""
    key = _key(over)
    if key not in run.reclustered:
        rc, labels, res = run.live.cluster(params_of(P, params, **over), len(run.pts))
        assert rc == 0, (run.frame, rc)
        labels.setflags(write=False)
        run.reclustered[key] = (labels, int(res.n_merges), int(res.n_regions), int(res.n_supervoxels))
    return run.reclustered[key]


# ------------------------------------------------------------------------------------------------ the mixes
Mix = collections.namedtuple("Mix", "name kind frames params env cond expect")
# frames: names of FRAMES, one per context, in context order;  env: the switches of the call (None: the variable is unset);  cond: the condition check_condition asserts;
# expect: what the GPU test has to observe besides "every frame equals the oracle" (by kind)
MIXES = []


def mix(name, kind, frames, params, env, cond, **expect):
    MIXES.append(Mix(name, kind, tuple(frames), params, env, cond, expect))


# 1. one deep frame beside shallow ones: the sorts of all frames are as wide as the deepest needs, the tile path is refused for all before anything ran (depth 17 and
#    more), the point sort moves (key, index) pairs for all (depth 18 and more).  The predicted path and sort form are part of the name: no observable tells which sort form ran.
DEPTH_PREDICTIONS = {      # (depth, F3DS_VOX_TILES) -> (stage0_path, sort form): what predict_stage0 has to give from the oracle's depths and point counts
    (13, None): ("tiles", None), (16, None): ("tiles", None), (17, None): ("sort", "one-word"), (18, None): ("sort", "pairs"), (21, None): ("sort", "pairs"),
    (13, "0"): ("sort", "one-word"), (16, "0"): ("sort", "one-word"), (17, "0"): ("sort", "one-word"), (18, "0"): ("sort", "pairs"), (21, "0"): ("sort", "pairs"),
}


def _depth_name(d, tiles, pred, wide=False):
    return "depth-%d%s-vox-tiles-%s-%s%s" % (d, "-wide" if wide else "", "unset" if tiles is None else tiles, pred[0], "-" + pred[1] if pred[1] else "")


for (_d, _t), _p in DEPTH_PREDICTIONS.items():
    mix(_depth_name(_d, _t, _p), "depth", ["one-point", "block3x1x1", "block8", "far%d" % _d], "default", dict(F3DS_VOX_TILES=_t), ("depths", (1, 2, 3, _d), 4096), path=_p[0], sort=_p[1])
# ... and with a deep frame of 4 097 .. 8 192 points: tile_bits and idxbits grow by one each, 3 * 17 + 1 + 13 = 65: pairs at depth 17 already
for _t in (None, "0"):
    mix(_depth_name(17, _t, ("sort", "pairs"), wide=True), "depth", ["one-point", "block3x1x1", "block8", "far17-wide"], "default", dict(F3DS_VOX_TILES=_t), ("depths", (1, 2, 3, 17), 8192), path="sort", sort="pairs")

# 2. a frame of one voxel beside a frame of 13 824: every kernel is launched as wide as the big frame needs, and its E moves every frame to global keys
SIZE_FRAMES = ["one-point", "block3x1x1", "count4097", "block24-random"]
mix("size-mix", "size", SIZE_FRAMES, "manual-2r", {}, ("sizes", 1000), layout=(8, 0), lone_layout=(8, 2), frames_in_shape=4, path="sort")
mix("size-mix-16", "size", SIZE_FRAMES * 4, "manual-2r", {}, ("sizes", 1000), layout=(8, 0), shape=(GRID_TARGET // 16, WIDE_CAP, 16), path="sort")

# 3. frames that leave the batch (no point, no finite point: both leave at the first drop_dead of stage 0): the owner among them, between live frames, all of them
mix("dead-owner-and-between", "dead", ["empty", "all-nan", "block8", "one-point", "all-nan", "block3x1x1"], "default", {}, ("dead", (0, 1, 4)))
mix("dead-all", "dead", ["empty", "all-nan", "empty", "all-nan"], "default", {}, ("dead", (0, 1, 2, 3)))
mix("dead-last", "dead", ["block8", "empty"], "default", {}, ("dead", (1,)))

# 4. the tile path refuses one frame (not the owner's) after it ran: all four run again on the sort path, and the batch stays off the tile path while that context waits
mix("tile-refusal-memory", "refusal", ["block8", "one-dense-257", "block3x1x1", "s-ordered"], "default", dict(F3DS_VOX_TILES=None, F3DS_TRACE_ERR="1"), ("one_dense", 1, 257))

# 5. one context with a short adjacency list: the pass of all four frames runs again, twice
REGROW_FRAMES = ["block12-random", "block8", "block3x1x1", "one-point"]
mix("adjacency-regrow-mix-short-first", "regrow", REGROW_FRAMES, "seed-r", dict(F3DS_TRACE_ERR="1"), ("regrow", 0, 2), short=0, reruns=2)
mix("adjacency-regrow-mix-short-last", "regrow", REGROW_FRAMES[1:] + REGROW_FRAMES[:1], "seed-r", dict(F3DS_TRACE_ERR="1"), ("regrow", 3, 2), short=3, reruns=2)

# 6. incident-list pools that overflow in two frames of four: the merge stage of all four runs again, the frame without an edge included
mix("merge-rerun-mix", "rerun", ["block3x1x1", "block14-random", "plane64-grey", "block8"], "manual-2r", dict(F3DS_ILIST_SLACK="1", F3DS_TRACE_ERR="1"), ("merges", 0, {1: 200, 2: 900}))

MIX = {m.name: m for m in MIXES}
assert len(MIX) == len(MIXES)
NAMES = [m.name for m in MIXES]
STATE_MIXES = [m.name for m in MIXES if m.kind in ("size", "regrow", "rerun")]      # the mixes after which every context is asked for its supervoxels, adjacency and a recluster


# every (frame, parameter set) a mix runs, and the two depths of the table that no mix takes: what the CPU test runs through the emulation
PAIRS = sorted({(f, m.params) for m in MIXES for f in m.frames} | {("far19", "default"), ("far20", "default")})


def runs_of(oracle, P, m):
    return [oracle_run(oracle, P, f, m.params) for f in m.frames]


def adjacency_room(S0, mult):
    return min(S0 * mult + EDGE_EXTRA, 0x7FFFFFFF)


def regrows_needed(E, S0, mult):
    """How often a frame of E adjacencies and S0 seeds overflows its list, starting from this multiplier."""
    k = 0
    while E > adjacency_room(S0, mult):
        mult *= EDGE_GROW; k += 1
    return k


# ------------------------------------------------------------------------------------------------ the conditions
def check_condition(m, runs):
    """Assert that the oracle's lone runs of a mix's frames meet the condition that makes the batch the mix it is named for."""
    what, args = m.cond[0], m.cond[1:]
    if what == "depths":               # the depths are the named ones; the deep frame alone is over the block table's depth; the prediction is the formulas'
        depths = tuple(int(r.res.octree_depth) for r in runs)
        n = [len(r.pts) for r in runs]
        assert depths == args[0] and [DEPTH_OF[f] for f in m.frames] == list(depths), depths
        assert args[1] // 2 < max(n) <= args[1] if args[1] > VT_TILE else max(n) <= VT_TILE, n      # (the widest frame: one tile and at most 12 index bits, or two and 13)
        tile_bits, idxbits = bits_for((max(n) + VT_TILE - 1) // VT_TILE - 1), bits_for(max(n) - 1)
        assert (tile_bits == 0 and idxbits <= 12) if args[1] == VT_TILE else (tile_bits, idxbits) == (1, 13), (tile_bits, idxbits)
        assert sum(d > N_BLOCK_DEPTH_MAX for d in depths) == 1 and depths[-1] > N_BLOCK_DEPTH_MAX
        assert all(r.census.max_points_per_voxel <= C.VL_MAX_RUN and r.census.max_tile_voxels <= C.VT_ENT_MAX for r in runs)      # (no refusal after the tile path ran)
        assert predict_stage0(depths, n, len(runs), m.env.get("F3DS_VOX_TILES")) == (m.expect["path"], m.expect["sort"])
    elif what == "sizes":
        V = [int(r.res.n_voxels) for r in runs]; E = [int(r.res.n_edges) for r in runs]
        assert min(V) == 1 and max(V) >= args[0] * min(V), V
        big = [v == max(V) for v in V]
        assert sum(big) == len(runs) // 4 and all((e > FIT_EDGES) == b for e, b in zip(E, big)), E      # the big frame's E alone is over the largest LDS fit
        # ... and it alone has tiles of more voxels than the tile path takes (a point per voxel: 4096 in a tile): the voxelisation of all frames runs again on the sort path
        assert all((r.census.max_tile_voxels > C.VT_ENT_MAX) == b and r.census.max_points_per_voxel <= C.VL_MAX_RUN for r, b in zip(runs, big))
        assert predict_batch_path(runs, len(runs)) == m.expect["path"] == "sort"
    elif what == "dead":
        assert tuple(i for i, r in enumerate(runs) if r.res.n_voxels == 0) == args[0]
        for i in args[0]:
            r = runs[i]
            assert (r.labels == 0xFFFFFFFF).all() and r.res.n_finite == 0 and r.res.n_regions == 0 and r.res.n_points == len(r.pts)
        assert runs[0].res.n_voxels == 0 or m.name == "dead-last"      # (the owner of the call is dead)
    elif what == "one_dense":          # exactly one frame, not the owner's, has a voxel over VL_MAX_RUN; nothing else is over a limit of stage 0
        ppv = [r.census.max_points_per_voxel for r in runs]
        assert ppv[args[0]] == args[1] > C.VL_MAX_RUN and all(p <= C.VL_MAX_RUN for i, p in enumerate(ppv) if i != args[0]) and args[0] != 0, ppv
        assert all(r.census.max_tile_voxels <= C.VT_ENT_MAX for r in runs)
        d = [int(r.res.octree_depth) for r in runs]; n = [len(r.pts) for r in runs]
        assert tile_key_bits(d, n) <= KEY_BITS and len(runs) >= TILE_MIN_FRAMES
    elif what == "regrow":             # the short context's frame overflows its list exactly args[1] times, no other frame overflows the default list
        short = args[0]
        for i, r in enumerate(runs):
            k = regrows_needed(int(r.res.n_edges), int(r.res.n_seeds), 1 if i == short else EDGE_MULT)
            assert k == (args[1] if i == short else 0), (r.frame, int(r.res.n_edges), int(r.res.n_seeds), k)
        r = runs[short]
        assert adjacency_room(int(r.res.n_seeds), EDGE_GROW) < r.res.n_edges <= adjacency_room(int(r.res.n_seeds), EDGE_GROW ** 2)
    elif what == "merges":             # one frame without an edge (its pool cannot overflow), the named frames with many merges
        assert runs[args[0]].res.n_edges == 0 and runs[args[0]].res.n_merges == 0
        for i, least in args[1].items():
            assert runs[i].res.n_merges >= least, (runs[i].frame, int(runs[i].res.n_merges))
    else:
        raise AssertionError("unknown condition %r" % (what,))
