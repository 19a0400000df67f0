"""Synthetic lattice clouds for the supervoxel half of the path (voxelisation, neighbour search, normals, seeds, the label-propagation sweeps, adjacency), and a census of
the oracle's run that says which data-dependent path of csrc/f3ds_kernels.inc a cloud reaches.

Plain numpy, no GPU, no files.  cloud() builds an N x 4 float32 frame whose points sit at (cell + offset) * res; census() reads the oracle's arrays alone (never the
code under test): the one-ring and two-ring sizes of every 128-voxel tile of d_normals_t, the most points of a voxel, the distinct voxels of every 4096-point tile of
stage 0, whether two runs of one voxel meet inside one 256-point step, the leaves of every supervoxel, S0, V and the sweep count.  CASES lists every cloud with the path
it is for and the condition (check_condition) its oracle run -- and, where sweeps are concerned, the emulation's sweep statistics -- has to meet for the case to exercise that
path: tests/test_vccs_clouds_cpu.py asserts every condition and that the emulation equals the oracle byte for byte, tests/test_vccs_clouds_gpu.py runs every case through
the HIP kernels.

Why lattices.  The golden frames are noisy surfaces: no 128-voxel tile of theirs has a one-ring of more than 347 voxels (NT_RING1 = 448) or a two-ring of more than 528
(NT_SLOTS = 896), no run of sweeps is longer than 56 (the memo tag wraps at 63), no voxel holds more than 25 points (VL_MAX_RUN = 256).  A solid block has 27 neighbours
per voxel, a one-cell corridor lets a label travel for a hundred sweeps, and a point count per cell is whatever the case asks for."""
import collections
import ctypes
import functools
import os
import re

import numpy as np

from conftest import ALL_DEBUG, first_mismatch

# ---- the constants of the kernels the cases are sized by (checked against the library's own by test_vccs_clouds_cpu.py)
NT_TILE = 128           # voxels per tile of d_normals_t (leaf order)
NT_RING1 = 448          # distinct voxels a tile's one-ring may hold (a ring of exactly 448 fits)
NT_SLOTS = 896          # ... and its two-ring
VL_MAX_RUN = 256        # points per voxel stage 0's tile path accepts
VT_TILE = 4096          # points per tile of stage 0's tile path
VT_ENT_MAX = 1280       # distinct voxels such a tile may hold (VT_TILE / 2 * 5 / 8)
VG_CHUNK = 1024         # points of the leaf lists that pass through LDS together
RL_LDS_CAP = 12288      # labels 0..S0 the one-kernel relabel keeps in LDS (S0 + 1 <= cap)
HT_CAP = 256            # entries of a helper's tile list (64-voxel tiles it has leaves in)
HT_ROW = 16             # tile-list entries a row-path helper may have in d_centroid / d_sv_fill
QL = 64                 # leaves a row-path helper may have in d_centroid
TAG_PERIOD = 63         # a_sweep_tag(t) = t % 63 + 1
R_STACK = 24            # F3DS_R_STACK: depth of the R walkers' explicit stack
R_ROUNDS = 4            # F3DS_R_ROUNDS
BY_WAVE_RATIO = 48      # d_centroid: V > 48 * S0 -> a wave per helper
TILE_NONE = 0xFFFFFFFF  # SW_TILE_NONE / Context.tile_list_lengths() of a tile that overflowed

KERNEL_CONSTANTS = {       # name of P.constant() -> the value the cases assume
    "NT_TILE": NT_TILE, "NT_RING1": NT_RING1, "NT_SLOTS": NT_SLOTS, "VL_MAX_RUN": VL_MAX_RUN, "VT_TILE": VT_TILE, "VT_TAB": VT_TILE // 2, "VT_ENT_MAX": VT_ENT_MAX,
    "VG_CHUNK": VG_CHUNK, "RL_LDS_CAP": RL_LDS_CAP, "HT_CAP": HT_CAP, "HT_ROW": HT_ROW, "QL": QL, "TAG_PERIOD": TAG_PERIOD, "R_STACK": R_STACK, "R_ROUNDS": R_ROUNDS,
    "BY_WAVE_RATIO": BY_WAVE_RATIO, "SW_TILE_NONE": TILE_NONE,
}
# The side of each limit the limit itself falls on, by the cases that sit on it from both sides (name of the limit -> (the case that still fits, the first that does not)):
# what the comparison operators of the kernels decide.  test_vccs_clouds_cpu.py asserts that the pairs are in the case list with the conditions that say so.
BOUNDARY_CASES = {
    "VL_MAX_RUN": ("s-voxel-of-256-points", "s-voxel-of-257-points"),       # e - s > VL_MAX_RUN: a voxel of exactly 256 points stays on the tile path
    "VT_ENT_MAX": ("s-tile-of-1280-voxels", "s-tile-of-1281-voxels"),       # the entry after the 1280th is refused (>=, counted from 0)
    "RL_LDS_CAP": ("r-every-voxel-a-seed-12287", "r-every-voxel-a-seed-12288"),
}
# The two limits no lattice block sits on from both sides (no block gives a largest one-ring of 443..455 with every two-ring fitting, nor a two-ring of 897..900): their
# comparisons are one-line predicates beside the constants, and these patterns are aimed at those definition lines of f3ds_kernels.inc.
PREDICATE_PATTERNS = [
    (r"__host__ __device__ constexpr bool nt_ring1_holds\(uint32_t sl\) \{ return sl (<) \(uint32_t\)NT_RING1; \}", "<"),
    (r"__host__ __device__ constexpr bool nt_slots_hold\(uint32_t sl\) \{ return sl (<) \(uint32_t\)NT_SLOTS; \}", "<"),
]


def read_predicates(csrc_dir):
    """[(pattern, operators found, operator expected)] of the predicate definitions above."""
    text = open(os.path.join(csrc_dir, "f3ds_kernels.inc")).read()
    return [(pat, re.findall(pat, text), want) for pat, want in PREDICATE_PATTERNS]


# ------------------------------------------------------------------------------------------------ the generator
def pack_rgb(r, g, b):
    return (np.asarray(r, np.uint32) << 16) | (np.asarray(g, np.uint32) << 8) | np.asarray(b, np.uint32)


GREY = int(pack_rgb(120, 130, 110))


def cloud(cells, res, rgba=GREY, per_cell=1, order="cell", nan_every=0, offset=0.5, seed=0, anchor=True):
    """N x 4 float32 frame: the points of cell (i, j, k) sit at (cell + offset) * res, a packed uint32 colour in column 3.
    cells: K x 3 integers;  rgba: one packed colour, K of them, or 'random' (per cell, from `seed`);  per_cell: points per cell, one number or K of them -- the first at
    `offset`, the others at offsets drawn in [0.25, 0.75)^3 (well inside the cell);  order: 'cell' (a cell's points side by side, cells as given), 'round' (the first point
    of every cell, then the second of every cell that has one, ...: the runs of a voxel lie far apart), 'shuffle' (a permutation drawn from `seed`);  nan_every = k > 0: a
    row of NaNs in front of every k-th point.
    anchor: two more points, the frame's last.  The voxel grid is a cube of 2^depth voxels CENTRED on the frame's bounding box, so where the voxel borders fall depends on
    the box: the anchors -- at offset 0.25 in the lowest cell of the cells' bounding box and at offset 0.75 in its highest, the box rounded up to an even number of cells
    per axis -- pin the box so that every voxel IS a cell and every point lies a quarter of a cell inside its voxel at the least (without them points sit on voxel
    borders, where float rounding decides their keys).  An anchor is one more point of its corner cell or, where that cell is empty, a voxel of its own.  Deterministic: the same arguments give the same bytes."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    K = len(cells)
    rng = np.random.default_rng(seed)
    if isinstance(rgba, str):
        assert rgba == "random"
        col = pack_rgb(*rng.integers(0, 256, (3, K)))
    else:
        col = np.broadcast_to(np.asarray(rgba, np.uint32), (K,))
    cnt = np.broadcast_to(np.asarray(per_cell, np.int64), (K,))
    owner = np.repeat(np.arange(K), cnt)
    first = np.zeros(K + 1, np.int64); first[1:] = np.cumsum(cnt)
    rank = np.arange(len(owner)) - first[:-1][owner]
    off = rng.uniform(0.25, 0.75, (len(owner), 3))
    off[rank == 0] = offset
    xyz = ((cells[owner] + off) * float(res)).astype(np.float32)
    if order == "round":
        perm = np.lexsort((owner, rank))
    elif order == "shuffle":
        perm = rng.permutation(len(owner))
    else:
        assert order == "cell"
        perm = np.arange(len(owner))
    pts = np.zeros((len(owner), 4), np.float32)
    pts[:, :3] = xyz[perm]
    pts[:, 3] = col[owner[perm]].astype(np.uint32).view(np.float32)
    if nan_every:
        at = np.arange(0, len(pts), nan_every)
        pts = np.insert(pts, at, np.full(4, np.nan, np.float32), axis=0)
    if anchor:
        lo = cells.min(axis=0)
        span = cells.max(axis=0) - lo + 1
        hi = lo + span + (span % 2) - 1
        a = np.zeros((2, 4), np.float32)
        a[0, :3] = ((lo + 0.25) * float(res)).astype(np.float32)
        a[1, :3] = ((hi + 0.75) * float(res)).astype(np.float32)
        a[:, 3] = np.uint32(GREY if isinstance(rgba, str) else col[0]).view(np.float32)
        pts = np.vstack([pts, a])
    return np.ascontiguousarray(pts)


def block(nx, ny, nz, at=(0, 0, 0)):
    """Every cell of an nx x ny x nz block, x fastest."""
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1) + np.asarray(at, np.int64)


def serpentine(rows, length, gap, width=1):
    """A corridor in the plane z = 0: `rows` rows of `length` cells, `width` cells wide, `gap` cells apart, joined at alternating ends."""
    cells = set()
    pitch = gap + width
    for r in range(rows):
        for x in range(length):
            for w in range(width):
                cells.add((x, r * pitch + w, 0))
        if r + 1 < rows:
            xs = range(length - width, length) if r % 2 == 0 else range(width)
            for x in xs:
                for y in range(r * pitch + width, (r + 1) * pitch):
                    cells.add((x, y, 0))
    return np.array(sorted(cells, key=lambda c: (c[1], c[0])), np.int64)


def lattice(n, pitch, dims=3):
    """n^dims isolated cells, `pitch` cells apart (pitch >= 2: no voxel has a neighbour)."""
    return block(n, n, n if dims == 3 else 1) * pitch


def comb(teeth, tooth_len, pitch=2):
    """A spine along x with a tooth of tooth_len cells along y at every `pitch`-th cell."""
    cells = [(x, 0, 0) for x in range(teeth * pitch)]
    for t in range(teeth):
        cells += [(t * pitch, y, 0) for y in range(1, tooth_len + 1)]
    return np.array(cells, np.int64)


# ------------------------------------------------------------------------------------------------ the census
Census = collections.namedtuple("Census", "V S0 S sweeps ring1 ring2 overflow fits full27 alone max_points_per_voxel tile_voxels max_tile_voxels disorder leaves n_points "
                                          "chunk_straddle first_last_tile helper_tiles disorder_runs")


def _ring_sizes(nbr):
    """Distinct voxels in the one-ring and in the two-ring of every tile of NT_TILE consecutive voxels (a voxel is its own neighbour: slot 13)."""
    V = len(nbr)
    tiles = (V + NT_TILE - 1) // NT_TILE
    r1 = np.zeros(tiles, np.int64); r2 = np.zeros(tiles, np.int64)
    for t in range(tiles):
        a = nbr[t * NT_TILE:(t + 1) * NT_TILE].ravel()
        one = np.unique(a[a >= 0])
        b = nbr[one].ravel()
        two = np.unique(b[b >= 0])
        r1[t] = len(one); r2[t] = len(two)
    return r1, r2


def census(P, handle, result, n_points=None):
    """What the oracle's run says about the paths the frame takes, from the oracle's arrays alone."""
    nbr = handle.get("VOXEL_NEIGHBORS").reshape(-1, 27)
    V = len(nbr)
    assert V == result.n_voxels
    ring1, ring2 = _ring_sizes(nbr)
    overflow = (ring1 > NT_RING1) | (ring2 > NT_SLOTS)
    present = (nbr >= 0).sum(axis=1)
    count = handle.get("VOXEL_COUNT")
    pv = handle.get("POINT_VOXEL")
    n = len(pv)
    ntiles = (n + VT_TILE - 1) // VT_TILE
    tile_vox = np.array([len(np.unique(pv[t * VT_TILE:(t + 1) * VT_TILE][pv[t * VT_TILE:(t + 1) * VT_TILE] >= 0])) for t in range(ntiles)], np.int64)
    # two runs of one voxel inside one 256-point step: a run is a stretch of equal voxels inside one 64-lane wave (run_of_lane works per wave)
    disorder, disorder_runs = False, 0
    idx = np.arange(n)
    head = (pv >= 0) & ((idx % 64 == 0) | (np.concatenate([[-2], pv[:-1]]) != pv))
    hs, hv = idx[head] // 256, pv[head]
    if len(hs):
        key = hs.astype(np.int64) * (V + 1) + hv
        disorder_runs = len(key) - len(np.unique(key))      # runs that meet an earlier run of their voxel in their step
        disorder = disorder_runs > 0
    sv = handle.get("VOXEL_SVLABEL")
    leaves = np.bincount(sv[sv != 0]) if (sv != 0).any() else np.zeros(0, np.int64)
    leaves = leaves[leaves > 0]
    # entries of a helper's tile list: the 64-voxel tiles (ordinal >> 6) it has leaves in
    lab_tile = np.unique(np.stack([sv[sv != 0].astype(np.int64), np.nonzero(sv != 0)[0] >> 6], axis=1), axis=0) if (sv != 0).any() else np.zeros((0, 2), np.int64)
    helper_tiles = np.bincount(lab_tile[:, 0]) if len(lab_tile) else np.zeros(0, np.int64)
    helper_tiles = helper_tiles[helper_tiles > 0]
    # the leaf lists in leaf order: voxel v takes places start[v] .. start[v + 1]; a voxel straddles a VG_CHUNK boundary of the 256-voxel block it is gathered with
    start = np.zeros(V + 1, np.int64); start[1:] = np.cumsum(count)
    straddle = False
    for vb in range(0, V, 256):
        p0 = start[vb]
        s, e = start[vb:min(vb + 256, V)] - p0, start[vb + 1:min(vb + 256, V) + 1] - p0
        straddle = straddle or bool(((s // VG_CHUNK) != ((e - 1) // VG_CHUNK)).any())
    fl = False
    if ntiles >= 2:
        a = pv[:VT_TILE]; b = pv[(ntiles - 1) * VT_TILE:]
        fl = len(np.intersect1d(a[a >= 0], b[b >= 0])) > 0
    return Census(V, int(result.n_seeds), int(result.n_supervoxels), int(result.sweeps), ring1, ring2, overflow, ~overflow, int((present == 27).sum()), int((present == 1).sum()),
                  int(count.max()) if V else 0, tile_vox, int(tile_vox.max()) if ntiles else 0, bool(disorder), leaves, n, bool(straddle), bool(fl), helper_tiles, int(disorder_runs))


# ------------------------------------------------------------------------------------------------ the emulation's run
EmulRun = collections.namedtuple("EmulRun", "rc labels res h stats deep cold")
SWEEP_STATS = 22      # F3DS_DBG_SWEEP_STATS: (full from their start, incremental, fallback, idle)
FULL, INCREMENTAL, FALLBACK, IDLE = 0, 1, 2, 3


def emul_run(emul, pts, prm, inc_shift=None, cold=False):
    """The emulation's run of a frame with F3DS_EMUL_INC_SHIFT = inc_shift (None: unset) and its sweep statistics.  deep: how often a walker the device runs too put a
    voxel off because its R chain overflowed the stack, in the emulation's own order (ascending ordinals, one voxel after the other).  cold (only with cold=True, which
    copies the memo once per voxel): voxels whose a_eval_R_mask overflows when it starts from the memo as the pre-pass left it."""
    old = {k: os.environ.pop(k, None) for k in ("F3DS_EMUL_INC_SHIFT", "F3DS_EMUL_R_COLD")}
    try:
        if inc_shift is not None:
            os.environ["F3DS_EMUL_INC_SHIFT"] = inc_shift
        if cold:
            os.environ["F3DS_EMUL_R_COLD"] = "1"
        rc, labels, res, h = emul.segment(pts, prm)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    stats, deep, ncold = None, None, None
    if rc == 0:
        buf = np.zeros(4, np.uint32); nb = ctypes.c_size_t()
        assert emul.fn("get")(h.h, SWEEP_STATS, ctypes.c_void_p(buf.ctypes.data), ctypes.c_size_t(16), ctypes.byref(nb)) == 0 and nb.value == 16
        stats = tuple(int(x) for x in buf)
        f = emul.fn("r_deep"); f.restype = ctypes.c_uint32
        deep = int(f(h.h))
        f = emul.fn("r_deep_cold"); f.restype = ctypes.c_uint32
        ncold = int(f(h.h)) if cold else None
    return EmulRun(rc, labels, res, h, stats, deep, ncold)


def emul_equals_oracle(er, olabels, oh):
    """None when the emulation's labels and every array of ALL_DEBUG equal the oracle's byte for byte, the first difference otherwise."""
    if not np.array_equal(er.labels, olabels):
        return "labels differ at %d points" % int((er.labels != olabels).sum())
    for w in ALL_DEBUG:
        m = first_mismatch(w, oh.get(w), er.h.get(w))
        if m:
            return m
    return None


# ------------------------------------------------------------------------------------------------ exact ties between two helpers
DP_VOXEL_DISTANCE = 15      # devprobe_inputs.FN["n_voxel_distance"]


def tie_count(hostprobe, handle, prm):
    """Voxels whose two smallest distances to the final helper centroids (the oracle's SV_CENTROID) are equal bit for bit, by the host build of n_voxel_distance
    (tests/devprobe): where the sweeps have to break a tie between two helpers by their order alone."""
    cen = handle.get("SV_CENTROID").reshape(-1, 10)[:, :9]
    vox = np.concatenate([handle.get("VOXEL_XYZ").reshape(-1, 3), handle.get("VOXEL_RGB").reshape(-1, 3), handle.get("VOXEL_NORMAL").reshape(-1, 4)[:, :3]], axis=1)
    S, V = len(cen), len(vox)
    if S < 2:
        return 0
    rows = np.zeros((V * S, 22), np.float32)
    rows[:, 0:9] = np.tile(cen, (V, 1))
    rows[:, 9:18] = np.repeat(vox, S, axis=0)
    rows[:, 18:22] = (prm.seed_res, prm.w_normal, prm.w_color, prm.w_spatial)
    d = hostprobe.run(DP_VOXEL_DISTANCE, rows.view(np.uint32)).view(np.float32).reshape(V, S)
    d = np.sort(d, axis=1)
    return int((d[:, 0].view(np.uint32) == d[:, 1].view(np.uint32)).sum())


# ------------------------------------------------------------------------------------------------ the cases
R = 0.01                # lattice pitch = voxel_res of most cases
RD = 1.0 / 64           # ... of the tie cases: every coordinate, sum and mean is a dyadic rational, so distances to two mirrored helpers are equal bit for bit
Case = collections.namedtuple("Case", "name family build params cond also_full")
# build: () -> frame (a lattice cloud; family 5: a frame of the library's synthetic generator);  params: overrides on top of --CVX --AL -t 0.2 with use_transform = 0;  cond: the condition the census / the emulation's statistics have to meet
# (check_condition);  also_full: the case runs once more with every sweep full (F3DS_INC_SHIFT = -1 / F3DS_EMUL_INC_SHIFT = -1)
CASES = []


def case(name, family, build, cond, also_full=False, **params):
    p = dict(voxel_res=R, seed_res=5 * R, use_transform=0)
    p.update(params)
    CASES.append(Case(name, family, build, p, cond, also_full))


def _with_far(cells, far):
    return np.vstack([cells, np.asarray(far, np.int64).reshape(-1, 3)])


def _one_dense(k, at=70):
    pc = np.ones(144, np.int64); pc[at] = k
    return cloud(block(12, 12, 1), R, per_cell=pc)


def _count_frame(n):
    """A frame of exactly n points (the two anchors included): 32 x 32 cells of four points, the first cells one more or less."""
    cells = block(32, 32, 1)
    pc = np.full(len(cells), 4, np.int64)
    d = n - 2 - int(pc.sum())
    pc[:abs(d)] += 1 if d > 0 else -1
    return cloud(cells, R, per_cell=pc)


def _cubes_and_crumbs():
    """Eight 4 x 4 x 4 cubes of 64 voxels, some a voxel more or less, 16 cells apart (a helper each at seed_res = 8 voxels), and forty 2 x 2 crumbs (a helper each): helpers
    of 64 and of 65 leaves in a frame whose mean supervoxel is small enough for the row path of d_centroid / d_sv_fill (V <= 48 S0)."""
    cells = []
    for i, sz in enumerate([63, 64, 65, 64, 65, 66, 64, 65]):
        o = np.array([(i % 4) * 16 + 1, (i // 4) * 16 + 1, 1])
        cells += [tuple(o + np.array([k % 4, (k // 4) % 4, k // 16])) for k in range(sz)]
    for i in range(40):
        o = np.array([(i % 8) * 8, (i // 8) * 8 + 40, 0])
        cells += [tuple(o + np.array(d)) for d in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0))]
    return cloud(np.array(cells), R, rgba="random")


# 1. normals tables (d_normals_t: NT_RING1 = 448, NT_SLOTS = 896; no block of 12..20 x 12..20 x 4..20 cells gives a largest two-ring of 897..900 or a largest one-ring of 443..447 / 449..455)
case("n-block8-all-fit", 1, lambda: cloud(block(8, 8, 8), R), ("all_fit", 200, 288))
case("n-ring2-896-fits", 1, lambda: cloud(block(18, 16, 18), R), ("all_fit", 428, 896))                  # a two-ring that fills the table exactly
case("n-ring2-901-over", 1, lambda: cloud(block(18, 12, 19), R), ("ring2_only", 422, 901))               # one-ring fits everywhere, one tile's two-ring does not
case("n-ring1-442-fits", 1, lambda: cloud(block(20, 19, 17), R), ("all_fit", 442, 892))
case("n-ring1-456-over", 1, lambda: cloud(block(17, 17, 17), R), ("ring1_only", 456, 859))               # one tile's one-ring does not fit, every two-ring would
case("n-block20x20x18-mix", 1, lambda: cloud(block(20, 20, 18), R), ("mix", 1, 2, 54))                  # (its tile with a one-ring of exactly 448 has a two-ring over 896: no block gave a 448 that fits)
case("n-block20-mix", 1, lambda: cloud(block(20, 20, 20), R), ("mix", 3, 17, 43))                        # one launch: 3 tiles over by their one-ring, 17 by their two-ring alone, 43 fit
case("n-block17-shifted", 1, lambda: cloud(_with_far(block(17, 17, 17), [(16, 21, -12), (21, 7, 9), (14, 0, 29)]), R), ("mix", 1, 4, 34))      # three far voxels move the block in Morton order: other tiles, other rings (458 / 1060)
for _v in (127, 128, 129, 257):
    case("n-line-V%d" % _v, 1, (lambda n: lambda: cloud(block(n, 1, 1), R))(_v - 1), ("V", _v))         # (the upper anchor is a voxel of its own); 129 and 257: a last tile of one voxel
case("n-isolated", 1, lambda: cloud(lattice(6, 3), R), ("alone", 216))
# 2. stage 0, tile path (forced by F3DS_VOX_TILES = 2 on the device)
for _k in (255, 256, 257):
    case("s-voxel-of-%d-points" % _k, 2, (lambda k: lambda: _one_dense(k))(_k), ("ppv", _k))
case("s-chunk-straddle", 2, lambda: cloud(block(8, 8, 1), R, per_cell=40), ("straddle",))
case("s-first-and-last-tile", 2, lambda: cloud(block(8, 8, 1), R, per_cell=130, order="round"), ("first_last",))
case("s-tile-of-1280-voxels", 2, lambda: cloud(block(40, 32, 1), R, per_cell=4, order="round"), ("tile_vox", 1280))
case("s-tile-of-1281-voxels", 2, lambda: cloud(_with_far(block(40, 32, 1), [(40, 0, 0)]), R, per_cell=4, order="round"), ("tile_vox", 1281))
case("s-shuffled", 2, lambda: cloud(block(16, 16, 2), R, per_cell=6, order="shuffle"), ("disorder", 500))      # (the lower anchor alone gives most clouds ONE such run)
case("s-ordered", 2, lambda: cloud(block(16, 16, 2), R, per_cell=4), ("disorder", 0))                         # (runs of four never straddle a wave; the anchors come 2048 points behind their cells)
case("s-nan-rows", 2, lambda: cloud(block(20, 20, 2), R, per_cell=3, nan_every=3), ("nan", 800))
case("s-4096-points", 2, lambda: _count_frame(4096), ("n_points", 4096))
case("s-4097-points", 2, lambda: _count_frame(4097), ("n_points", 4097))
# 3. exact ties between two helpers (uniform colour, seed spacing a whole number of voxels, dyadic coordinates)
case("t-plane24", 3, lambda: cloud(block(24, 24, 1), RD), ("ties", 9), voxel_res=RD, seed_res=8 * RD)
case("t-block12", 3, lambda: cloud(block(12, 12, 12), RD), ("ties", 72), voxel_res=RD, seed_res=4 * RD)
# 4. long runs of sweeps (the memo tag wraps at 63 and again at 126)
case("w-corridor-ratio40", 4, lambda: cloud(serpentine(6, 40, 3), R), ("long", 63, 64), also_full=True, seed_res=40 * R)
case("w-corridor-ratio72", 4, lambda: cloud(serpentine(8, 40, 3), R), ("long", 126, 127), also_full=True, seed_res=72 * R)
case("w-wide-corridor-ratio40", 4, lambda: cloud(serpentine(8, 60, 3, width=3), R, rgba="random"), ("long", 63, 64), also_full=True, seed_res=40 * R)
case("w-wide-corridor-ratio72", 4, lambda: cloud(serpentine(8, 60, 3, width=3), R, rgba="random"), ("long", 126, 127), also_full=True, seed_res=72 * R)
case("w-early-fixed-point", 4, lambda: cloud(block(6, 6, 6), R), ("idle", 60), also_full=True, seed_res=40 * R)
# 5. deep chains without switches.  No lattice reaches them -- rods, planes, slabs, solid and sparse blocks at seed / voxel = 1.1 .. 4 in both leaf orders, with and without the
#    transform: at most the emulation's own cross-check (a_eval_R from an empty memo) overflows, on the plane of r-tiny-supervoxels-desc below -- but a small noisy surface
#    under the single-camera transform does: the sheet it becomes in (x / z, y / z, log z) has two voxels in three as seeds at seed / voxel = 2, and labels that fall along
#    paths of more than 24 of them.  (No cloud within the size limit made a sweep fall back at the default F3DS_R_ROUNDS: DESIGN.md 7.)
def _noisy_sheet():
    from conftest import pkg
    return pkg().synth_frame(0, 300328, 60, 40, 0)      # (the library's deterministic SplitMix64 generator: a 60 x 40 RGB-D frame, no holes)


case("d-deep-chain-desc", 5, _noisy_sheet, ("deep",), voxel_res=0.03, seed_res=0.06, use_transform=1, leaf_order=1)        # the walkers put 242 voxels off even in the emulation's order
case("d-deep-chain-cold", 5, _noisy_sheet, ("deep_cold",), voxel_res=0.03, seed_res=0.06, use_transform=1)                 # ... here only when no earlier voxel has memoised the chain (273)
case("r-tiny-supervoxels-desc", 6, lambda: cloud(block(40, 40, 1), R), ("no_deep", 400), seed_res=2 * R, leaf_order=1)
# 6. extremes of the seed ratio
for _s in (12287, 12288, 12289):
    case("r-every-voxel-a-seed-%d" % _s, 6, (lambda n: lambda: cloud(lattice(24, 3)[:n - 1], R))(_s), ("s0", _s), seed_res=R)      # RL_LDS_CAP: labels 0..S0 fit while S0 + 1 <= 12288
case("r-one-seed", 6, lambda: cloud(block(10, 10, 3), R, rgba="random"), ("one_seed",), seed_res=50 * R)
case("r-small-supervoxels", 6, lambda: cloud(block(32, 32, 1), R, rgba="random"), ("by_wave", False), seed_res=4 * R)
case("r-big-supervoxels", 6, lambda: cloud(block(32, 32, 1), R, rgba="random"), ("by_wave", True), seed_res=10 * R)
case("r-helpers-of-64-and-65-leaves", 6, _cubes_and_crumbs, ("leaves", 64, 65), seed_res=8 * R)
# (helpers with exactly 16 tile-list entries were not reached on the row path: this slab has helpers with 15 and with 17, the most any scanned frame with V <= 48 S0 gave,
# and V = 48 S0 exactly -- the last frame that takes the row path)
case("r-tile-lists-of-15-and-17", 6, lambda: cloud(block(24, 24, 6), R, rgba="random", seed=3), ("tile_entries", 15, 17), seed_res=4.5 * R)
# 7. variants: one case per family with descending leaves, one under the single-camera transform, one deep grid (the per-voxel neighbour table)
case("v-desc-ring1-456-over", 1, lambda: cloud(block(17, 17, 17), R), ("some_over_some_fit",), leaf_order=1)
case("v-desc-shuffled", 2, lambda: cloud(block(16, 16, 2), R, per_cell=6, order="shuffle"), ("disorder", 500), leaf_order=1)
case("v-desc-block12-ties", 3, lambda: cloud(block(12, 12, 12), RD), ("ties", 1), voxel_res=RD, seed_res=4 * RD, leaf_order=1)
case("v-desc-corridor-ratio40", 4, lambda: cloud(serpentine(6, 40, 3), R), ("long", 63, 64), also_full=True, seed_res=40 * R, leaf_order=1)
case("v-desc-big-supervoxels", 6, lambda: cloud(block(32, 32, 1), R, rgba="random"), ("by_wave", True), seed_res=10 * R, leaf_order=1)
case("v-transform", 7, lambda: cloud(block(12, 12, 12, at=(50, 50, 100)), R), ("depth_at_most", 12), use_transform=1)
case("v-depth13", 7, lambda: cloud(_with_far(block(8, 8, 8), [(5000, 3000, 100)]), R), ("depth", 13))

CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)
NAMES = [c.name for c in CASES]
FAMILY_NAMES = {1: "normals tables", 2: "stage 0 tile path", 3: "exact ties", 4: "long runs of sweeps", 5: "deep chains", 6: "seed ratio extremes", 7: "variants"}


@functools.lru_cache(maxsize=None)
def frame_of(name):
    pts = CASE[name].build()
    pts.setflags(write=False)
    return pts


def params_of(P, name):
    return P.launch_params(**CASE[name].params)


Run = collections.namedtuple("Run", "case pts prm labels res h census seconds")
_runs, _emul_runs = {}, {}


def oracle_run(oracle, P, name):
    """The oracle's run of a case and its census, made once per process and shared (read-only) by every test that needs it."""
    if name not in _runs:
        import time
        pts, prm = frame_of(name), params_of(P, name)
        t0 = time.perf_counter()
        rc, labels, res, h = oracle.segment(pts, prm)
        dt = time.perf_counter() - t0
        assert rc == 0, "the oracle refuses case %s: %d" % (name, rc)
        _runs[name] = Run(CASE[name], pts, prm, labels, res, h, census(P, h, res), dt)
    return _runs[name]


def emul_run_of(emul, P, name, inc_shift=None):
    key = (name, inc_shift)
    if key not in _emul_runs:
        _emul_runs[key] = emul_run(emul, frame_of(name), params_of(P, name), inc_shift, cold=CASE[name].cond[0] in ("deep", "deep_cold", "no_deep"))
    return _emul_runs[key]


def predicted_stage0(cen, depth):
    """What Context.stage0_path() has to say when the tile path is forced: it refuses a voxel of more than VL_MAX_RUN points and a tile of more than VT_ENT_MAX voxels."""
    return "tiles" if cen.max_points_per_voxel <= VL_MAX_RUN and cen.max_tile_voxels <= VT_ENT_MAX else "sort"


# ------------------------------------------------------------------------------------------------ the conditions
def check_condition(r, er, ties=None):
    """Assert that the oracle's run r of a case (and the emulation's run er of it, where sweeps are concerned) meets the condition that makes the case exercise its path.
    ties: tie_count() of the run, for the tie cases."""
    c, cen = r.case, r.census
    what, args = c.cond[0], c.cond[1:]
    over1 = int((cen.ring1 > NT_RING1).sum()); over2 = int(((cen.ring1 <= NT_RING1) & (cen.ring2 > NT_SLOTS)).sum())
    assert cen.V <= 20000 and len(cen.ring1) == (cen.V + NT_TILE - 1) // NT_TILE
    assert er.stats is not None and sum(er.stats) == cen.sweeps
    if what == "all_fit":              # every tile fits; the largest rings are the ones the case is named for; interior voxels with all 27 slots present exist
        assert not cen.overflow.any() and (int(cen.ring1.max()), int(cen.ring2.max())) == args and cen.full27 > 0, (cen.ring1.max(), cen.ring2.max())
    elif what == "ring2_only":         # no one-ring overflows, exactly one tile's two-ring does
        assert over1 == 0 and over2 == 1 and (int(cen.ring1.max()), int(cen.ring2.max())) == args, (over1, over2, cen.ring1.max(), cen.ring2.max())
    elif what == "ring1_only":         # exactly one tile's one-ring overflows, and no two-ring would
        assert over1 == 1 and over2 == 0 and (int(cen.ring1.max()), int(cen.ring2.max())) == args and int(cen.ring2.max()) <= NT_SLOTS, (over1, over2, cen.ring1.max(), cen.ring2.max())
    elif what == "mix":
        assert (over1, over2, int(cen.fits.sum())) == args, (over1, over2, int(cen.fits.sum()))
    elif what == "some_over_some_fit":
        assert cen.overflow.any() and cen.fits.any()
    elif what == "V":                  # the tile edges: V = 127, 128, 129 (a last tile of one voxel), 257
        assert cen.V == args[0] and not cen.overflow.any()
    elif what == "alone":              # voxels without any neighbour (their own slot is the only one present)
        assert cen.alone >= args[0]
    elif what == "ppv":
        assert cen.max_points_per_voxel == args[0] and cen.max_tile_voxels <= VT_ENT_MAX
        assert predicted_stage0(cen, r.res.octree_depth) == ("tiles" if args[0] <= VL_MAX_RUN else "sort")
    elif what == "straddle":
        assert cen.chunk_straddle and cen.n_points > 2 * VG_CHUNK and predicted_stage0(cen, 0) == "tiles"
    elif what == "first_last":
        assert cen.first_last_tile and cen.n_points > 2 * VT_TILE and cen.disorder and predicted_stage0(cen, 0) == "tiles"
    elif what == "tile_vox":
        assert cen.max_tile_voxels == args[0] and cen.max_points_per_voxel <= VL_MAX_RUN
        assert predicted_stage0(cen, 0) == ("tiles" if args[0] <= VT_ENT_MAX else "sort")
    elif what == "disorder":           # runs of a voxel that meet an earlier run of it inside one 256-point step: none, or so many that the anchors cannot account for them
        assert (cen.disorder_runs >= args[0] if args[0] else cen.disorder_runs == 0) and cen.disorder == (args[0] > 0) and predicted_stage0(cen, 0) == "tiles", cen.disorder_runs
    elif what == "nan":
        nan_rows = int(np.isnan(r.pts[:, 0]).sum())
        assert nan_rows >= args[0] and int(r.res.n_finite) == len(r.pts) - nan_rows and predicted_stage0(cen, 0) == "tiles"
    elif what == "n_points":
        assert cen.n_points == args[0] == len(r.pts) and predicted_stage0(cen, 0) == "tiles"
    elif what == "ties":
        assert ties is not None and ties >= 1 and ties >= args[0], ties
    elif what == "long":               # more sweeps than the tag has values (twice over), and more of them busy than that
        busy = er.stats[FULL] + er.stats[INCREMENTAL] + er.stats[FALLBACK]
        assert cen.sweeps > args[0] and busy > args[1], (cen.sweeps, er.stats)
    elif what == "idle":
        assert er.stats[IDLE] >= args[0] > 0 and cen.sweeps > TAG_PERIOD, er.stats
    elif what == "deep":               # a walker the device runs too (a_eval_R_mask behind the pre-pass) overflows F3DS_R_STACK and puts voxels off, in the emulation's order
        assert er.deep > 0 and er.cold >= 1 and er.stats[FALLBACK] == 0, (er.deep, er.cold)
    elif what == "deep_cold":          # ... only from the memo as the pre-pass left it: whether the device puts a voxel off depends on the order its threads run in
        assert er.deep == 0 and er.cold > R_STACK, (er.deep, er.cold)
    elif what == "no_deep":            # tiny supervoxels; and the recorded fact that no walker the device runs overflows its stack here (a cloud that does belongs to family 5)
        assert cen.S0 >= args[0] and cen.V <= BY_WAVE_RATIO * cen.S0 and (er.deep, er.cold) == (0, 0), (cen.S0, er.deep, er.cold)
    elif what == "tile_entries":       # entries of the helpers' tile lists in d_sv_fill (64-voxel tiles a helper has leaves in): the row path takes 16 at the most
        ht = cen.helper_tiles
        assert all(int((ht == k).sum()) >= 1 for k in args) and int(ht.max()) == max(args) == HT_ROW + 1 and min(args) == HT_ROW - 1 and not (ht == HT_ROW).any(), sorted(ht)[-6:]
        assert cen.V == BY_WAVE_RATIO * cen.S0, (cen.V, cen.S0)
    elif what == "s0":
        assert cen.S0 == cen.V == args[0] and cen.sweeps == 0, (cen.S0, cen.V, cen.sweeps)
    elif what == "one_seed":
        assert cen.S0 == 1 and r.res.n_edges == 0 and r.res.n_merges == 0 and r.res.n_regions == 1
    elif what == "by_wave":            # d_centroid / d_sv_fill: four helpers per wave while V <= 48 S0, a wave per helper beyond
        assert (cen.V > BY_WAVE_RATIO * cen.S0) == args[0] and cen.S0 > 4, (cen.V, cen.S0)
    elif what == "leaves":
        assert all(int((cen.leaves == k).sum()) >= 1 for k in args) and args == (QL, QL + 1) and cen.V <= BY_WAVE_RATIO * cen.S0, (sorted(cen.leaves)[-9:], cen.V, cen.S0)
    elif what == "depth":
        assert r.res.octree_depth == args[0] > 12
    elif what == "depth_at_most":
        assert r.res.octree_depth <= args[0] and r.prm.use_transform == 1
    else:
        raise AssertionError("unknown condition %r" % (what,))
