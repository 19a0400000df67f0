"""Synthetic clouds for the seed stage (selectInitialSupervoxelSeeds: d_chunkbox, d_seed_grow, d_seed_keys, d_cell_hash, d_seed_nn, d_seed_filter, d_seed_compact), a
brute-force reference of the stage in plain numpy, and a census -- taken from the reference alone -- that says which branch of the seed kernels a cloud reaches.

The reference restates the prose of oracle/f3ds_oracle.cpp::select_seeds and SURVEY.md Appendix A6, not the kernels' headers.  Where the oracle (and the kernels) search the
3 x 3 x 3 block of seed cells around a cell, the reference searches ALL voxels: the nearest voxel to every cell centre, and the voxels inside the radius of every seed voxel.
That the two agree on every cloud here is the check that the 27-cell restriction is sound; the kernels carry two further shortcuts (the own-cell shortcut of d_seed_nn, the
cell pruning of d_seed_filter) which neither the oracle nor tests/emul has, and families B, C and D are built around their margins.

Geometry of the lattice cases.  seed_frame() places voxels at positions q (in voxels, multiples of 1/16) relative to the frame's first voxel, which it pins to the lower
corner of the cloud.  The seed octree starts as the cube [q0 - m, q0 + m) around that voxel (m = seed_res / voxel_res) and grows by whole cubes, so seed cell j covers
q in [j m, (j + 1) m) on every axis and has its centre at (j + 1/2) m.  With voxel_res = 2^-6 every coordinate, difference, square and sum below is a dyadic rational that
float32 holds exactly: ties and the bounds r^2 and res^2 / 4 are hit bit for bit."""
import collections
import functools
import math

import numpy as np

import vccs_clouds_common as V
from conftest import ALL_DEBUG, first_mismatch

# ---- the constants of the seed kernels the cases are sized by (checked against the library's own by test_seed_clouds_cpu.py)
SEED_CHUNK = 256            # voxels per box of d_chunkbox; d_seed_grow looks at 256 chunk boxes per trip
CAND_STRIDE = 256           # list entries a wave of d_seed_nn / d_seed_filter takes per round
CELLS_PER_WG = 4            # seed cells per workgroup of d_seed_nn / d_seed_filter (a wave each)
MAX_SEED_EVENTS = 48        # F3DS_MAX_SEED_EVENTS
NN_MARGIN = 1e-3            # d_seed_nn: own-cell shortcut below res^2 / 4 * (1 - 1e-3) (less what the float centre can be off by)
PRUNE_MARGIN = 1.001        # d_seed_filter: a cell is looked up when its box is within r2 * 1.001 of the seed voxel
FLT_EPS = float(np.finfo(np.float32).eps)

SEED_ULP = 2.0 ** -23       # d_seed_nn: the half cell gives up this much of the centre's largest coordinate before it is squared
SEED_CONSTANTS = {       # name of P.constant() -> the value the cases assume
    "SEED_CHUNK": SEED_CHUNK, "d_seed_grow::BLOCK": SEED_CHUNK, "SEED_CAND_STRIDE": CAND_STRIDE, "SEED_CELLS_PER_WG": CELLS_PER_WG, "d_seed_nn::BLOCK": 64 * CELLS_PER_WG,
    "d_seed_filter::BLOCK": 64 * CELLS_PER_WG, "MAX_SEED_EVENTS": MAX_SEED_EVENTS, "SEED_NN_MARGIN": NN_MARGIN, "SEED_NN_ULP": SEED_ULP, "SEED_PRUNE_MARGIN": PRUNE_MARGIN,
}
# The two strict comparisons of d_seed_filter, by the cases that sit on them from both sides (test_seed_clouds_cpu.py asserts they are in the list; their conditions in
# check_condition say what they hold): (float)num > min_points -- c9-min-points-exactly-2 has seeds with exactly min_points = 2 neighbours (dropped) and with more (kept);
# a_sqdist < r2 -- c2-at-the-radius has voxels at exactly the radius (not counted) beside voxels inside it (counted), both deciding whether a seed is kept.
FILTER_BOUNDARY_CASES = {"num > min_points": "c9-min-points-exactly-2", "a_sqdist < r2": "c2-at-the-radius"}


# ------------------------------------------------------------------------------------------------ the reference
f32 = np.float32
Event = collections.namedtuple("Event", "trigger depth lower upper edge min off")      # lower / upper: the axes on which the trigger lay below / at or above the cube; edge: inside [max, max + FLT_EPS) on some axis; min, off: the cube minimum and the key shift after the event
Grid = collections.namedtuple("Grid", "min depth res keys events")


def grow_grid(xyz, seed_res):
    """adoptBoundingBoxToPoint over the voxel centroids in leaf order, in float64: the final cube minimum, its depth, every voxel's key with the shifts of the later events
    applied, and the events.  Between two events the cube does not change, so the next voxel outside it is looked for in one vectorised pass; what happens at that voxel is
    the literal loop."""
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    n = len(p)
    res = float(f32(seed_res))
    keys = np.zeros((n, 3), np.int64)
    mn = np.zeros(3); mx = np.zeros(3)
    depth, defined, events, i = 0, False, [], 0
    off = [0, 0, 0]
    while i < n:
        if defined:
            bad = np.nonzero(((p[i:] < mn) | (p[i:] >= mx)).any(axis=1))[0]
            j = i + int(bad[0]) if len(bad) else n
            keys[i:j] = ((p[i:j] - mn) / res).astype(np.int64)      # (truncation of a non-negative quotient)
            i = j
            if i == n:
                break
        pt = p[i]
        while True:
            lo = pt < mn; up = pt >= mx
            if not (lo.any() or up.any() or not defined):
                break
            if defined:
                edge = bool(((pt >= mx) & (pt < mx + FLT_EPS)).any())
                side = float(1 << depth) * res
                for a in range(3):
                    if not up[a]:
                        mn[a] -= side
                        keys[:i, a] += 1 << depth      # the old root becomes the upper child
                        off[a] += 1 << depth
                depth += 1
                assert depth <= 21
                side = float(1 << depth) * res - FLT_EPS
                mx = mn + side
                events.append(Event(i, depth, tuple(bool(x) for x in lo), tuple(bool(x) for x in up), edge, tuple(float(x) for x in mn), tuple(off)))
            else:
                mn = pt - res / 2; mx = pt + res / 2
                mk = max(int(math.ceil((mx[a] - mn[a] - FLT_EPS) / res)) for a in range(3))
                depth = int(math.ceil(math.log(max(mk, 2)) / math.log(2.0) - FLT_EPS))
                side = float(1 << depth) * res
                for a in range(3):
                    over = (side - (mx[a] - mn[a])) / 2.0
                    if over > FLT_EPS:
                        mn[a] -= over; mx[a] += over
                defined = True
                events.append(Event(i, depth, (False,) * 3, (False,) * 3, False, tuple(float(x) for x in mn), tuple(off)))
        keys[i] = ((pt - mn) / res).astype(np.int64)
        i += 1
    return Grid(mn.copy(), depth, res, keys, events)


def morton(keys, depth):
    k = np.asarray(keys, np.uint64)
    code = np.zeros(len(k), np.uint64)
    for b in range(depth - 1, -1, -1):
        bb = np.uint64(b)
        code = (code << np.uint64(3)) | (((k[:, 0] >> bb) & np.uint64(1)) << np.uint64(2)) | (((k[:, 1] >> bb) & np.uint64(1)) << np.uint64(1)) | ((k[:, 2] >> bb) & np.uint64(1))
    return code


def sqdist(a, b):
    """flann::L2_Simple<float>: float32 operation by operation, the additions in the order x, y, z.  a: 3 floats, b: n x 3."""
    a = np.asarray(a, f32); b = np.asarray(b, f32)
    d = a[0] - b[:, 0]; r = d * d
    d = a[1] - b[:, 1]; r = r + d * d
    d = a[2] - b[:, 2]; r = r + d * d
    return r


def radius_sq(seed_res):
    return f32(float(f32(0.5) * f32(seed_res)) ** 2)


def min_points(seed_res, voxel_res):
    sr = f32(0.5) * f32(seed_res)
    return f32(0.05) * sr * sr * f32(3.1415926536) / (f32(voxel_res) * f32(voxel_res))


Ref = collections.namedtuple("Ref", "grid cell_keys cell_of centres seed_orig seed_dist keep seed_kept num r2 min_points")


def reference(xyz, seed_res, voxel_res):
    """The seed stage by brute force: the grid, the occupied cells in Morton order, the nearest voxel to every cell centre over ALL voxels under (distance, ordinal), and the
    filter with the radius counted over ALL voxels."""
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    g = grow_grid(xyz, seed_res)
    code = morton(g.keys, g.depth)
    ucode, first, cell_of = np.unique(code, return_index=True, return_inverse=True)
    cell_keys = g.keys[first]
    centres = ((cell_keys.astype(np.float64) + 0.5) * g.res + g.min).astype(f32)
    C = len(ucode)
    seed_orig = np.zeros(C, np.int32); seed_dist = np.zeros(C, f32)
    for c in range(C):
        d = sqdist(centres[c], xyz)
        seed_orig[c] = int(np.argmin(d))       # (the first of equal minima: the lowest ordinal)
        seed_dist[c] = d[seed_orig[c]]
    r2, mp = radius_sq(seed_res), min_points(seed_res, voxel_res)
    num = np.array([int((sqdist(xyz[s], xyz) < r2).sum()) for s in seed_orig], np.int64)
    keep = num.astype(f32) > mp
    return Ref(g, cell_keys, cell_of.reshape(-1), centres, seed_orig, seed_dist, keep, seed_orig[keep], num, r2, mp)


# ------------------------------------------------------------------------------------------------ the census
CellCensus = collections.namedtuple("CellCensus", "n_own n_block own_min shortcut other_cell tied tie_cells tie_winner_other kept_cells pruned_occupied counted_cells margin at_r2 "
                                                  "prune_slack")
Census = collections.namedtuple("Census", "V C cells events chunk_pos ref")


def shortcut_bound(res):
    """The bound the own-cell shortcut of d_seed_nn had before the centre's rounding was taken off it: every cell the kernel may take the shortcut in is under it."""
    return f32(0.25 * res * res * (1.0 - NN_MARGIN))


def census(xyz, seed_res, voxel_res, ref=None):
    """Per cell, from the reference alone: voxels in the cell and in its 27-block; the own-cell minimum and whether it is under the shortcut bound; whether the brute-force
    nearest voxel lies in another cell; whether the minimum is tied, across which cells, and whether the winner (the lowest ordinal) lies in another cell; how many of the 27
    cells around the seed voxel the filter's pruning rule keeps, how many occupied ones it prunes, in how many cells counted voxels lie; num - floor(min_points); whether a
    voxel lies at exactly r2; the least (box distance^2 / r2) over cells that hold a counted voxel.  Per frame: the events and where each trigger sits in its chunk."""
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    ref = ref or reference(xyz, seed_res, voxel_res)
    g = ref.grid
    by_key = {tuple(k): c for c, k in enumerate(ref.cell_keys.tolist())}
    members = [np.nonzero(ref.cell_of == c)[0] for c in range(len(ref.cell_keys))]
    near = shortcut_bound(g.res)
    x64 = xyz.astype(np.float64)
    cells = []
    for c, key in enumerate(ref.cell_keys.tolist()):
        own = members[c]
        block = [by_key[(key[0] + dx, key[1] + dy, key[2] + dz)] for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (key[0] + dx, key[1] + dy, key[2] + dz) in by_key]
        d_all = sqdist(ref.centres[c], xyz)
        own_min = d_all[own].min()
        tied = np.nonzero(d_all == ref.seed_dist[c])[0]
        tie_cells = sorted({int(ref.cell_of[t]) for t in tied})
        s = int(ref.seed_orig[c])
        skey = g.keys[s]
        kept, pruned_occ, slack = 0, 0, np.inf
        dd = sqdist(xyz[s], xyz)
        counted = np.nonzero(dd < ref.r2)[0]
        counted_cells = {int(ref.cell_of[t]) for t in counted}
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    far2 = 0.0
                    for a, dlt in enumerate((dx, dy, dz)):
                        lo = g.min[a] + float(skey[a]) * g.res
                        t = x64[s, a] - lo if dlt < 0 else ((lo + g.res) - x64[s, a] if dlt > 0 else 0.0)
                        far2 += max(t, 0.0) ** 2
                    k2 = (int(skey[0]) + dx, int(skey[1]) + dy, int(skey[2]) + dz)
                    if min(k2) < 0:
                        continue
                    if far2 <= float(ref.r2) * PRUNE_MARGIN:
                        kept += 1
                    elif k2 in by_key:
                        pruned_occ += 1
                    if k2 in by_key and by_key[k2] in counted_cells and (dx, dy, dz) != (0, 0, 0):
                        slack = min(slack, far2 / float(ref.r2))
        cells.append(CellCensus(len(own), int(sum(len(members[b]) for b in block)), own_min, bool(own_min < near), bool(ref.cell_of[s] != c), len(tied) > 1, tie_cells,
                                len(tied) > 1 and bool(ref.cell_of[s] != c), kept, pruned_occ, len(counted_cells), int(ref.num[c]) - int(math.floor(float(ref.min_points))),
                                bool((dd == ref.r2).any()), slack))
    return Census(len(xyz), len(cells), cells, g.events, [e.trigger % SEED_CHUNK for e in g.events], ref)


# ------------------------------------------------------------------------------------------------ the generator
RD = V.RD          # 2^-6: the voxel_res of every lattice case


def seed_frame(q, anchor_gap=4):
    """A frame whose voxels sit at the positions q (n x 3, in voxels, multiples of 1/16, all >= 0) relative to its first voxel, one point per voxel.  The first voxel is
    the lower corner: cell (0, 0, 0) at offset 1/4, where it is the lower anchor of the voxel grid as cloud() would place it; the upper anchor is a voxel of its own beyond every other.  A voxel at q lies in cell
    floor(q + 1/4); its offset in the cell has to stay within [1/8, 7/8]."""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    assert (q >= 0).all() and (q * 16 == np.round(q * 16)).all()
    cells = np.floor(q + 0.25).astype(np.int64)
    off = q + 0.25 - cells
    assert (off >= 0.125).all() and (off <= 0.875).all()
    origin = (cells == 0).all(axis=1)
    if origin.any():
        assert (off[origin] == 0.25).all()
    else:
        cells = np.vstack([[[0, 0, 0]], cells]); off = np.vstack([[[0.25] * 3], off])
    assert len(np.unique(cells, axis=0)) == len(cells), "two positions in one voxel"
    span = cells.max(axis=0) + 1
    hi = span + (span % 2) - 1
    if (cells == hi).all(axis=1).any():
        hi = hi + 2
    hi = hi + 2 * anchor_gap      # (anchor_gap: cells between the cloud and the upper anchor, so that it neither joins a cell nor counts in a radius)
    lim = ((cells == 0) & (off < 0.25)) | ((cells == hi) & (off > 0.75))
    assert not lim.any(), "a point outside the anchors' box"
    return V.cloud(np.vstack([cells, [hi]]), RD, offset=np.vstack([off, [[0.75] * 3]]), anchor=False)


def grid3(xs, ys=None, zs=None):
    ys = xs if ys is None else ys; zs = xs if zs is None else zs
    return np.array([(x, y, z) for x in xs for y in ys for z in zs], np.float64)


def cell_slots(m, origin, n=None, hollow=None):
    """The voxel positions of seed cell `origin` (a cell index per axis): slot (i, j, k) at q = origin m + (i, j, k) + 1/4, x fastest; the first n of them; hollow = r: without those nearer than r to the centre."""
    o = np.asarray(origin, np.float64) * m
    pts = np.array([(i, j, k) for k in range(m) for j in range(m) for i in range(m)], np.float64) + 0.25
    if hollow is not None:
        pts = pts[((pts - m / 2.0) ** 2).sum(axis=1) >= hollow * hollow]
    return (pts if n is None else pts[:n]) + o


# ---- family D: large offsets.  Built in two passes: the grid of a draft cloud (voxels at the nominal centres) tells where the float centres fall, the second pass places the voxels against them.
def _axis_hit(grid, key, centre, axis):
    """For cell `key` and its float centre: the nearest float beyond the upper face on `axis` (level with the centre otherwise), the nearest below the lower face's
    far side, and the own-cell voxel to go with it -- on the opposite side, its squared float32 distance just under the bound 0.25 res^2 (1 - 1e-3).  Returns (other, own)
    for the side on which the other cell's voxel comes nearest to the centre."""
    res = grid.res
    out = []
    for sign in (1, -1):
        face = grid.min[axis] + (key[axis] + (1 if sign > 0 else 0)) * res
        p = f32(face)
        if sign > 0:
            while ((float(p) - grid.min[axis]) / res) < key[axis] + 1:
                p = np.nextafter(p, f32(np.inf))
        else:
            while not ((float(p) - grid.min[axis]) / res) < key[axis]:
                p = np.nextafter(p, f32(-np.inf))
        other = centre.copy(); other[axis] = p
        out.append((float(sqdist(centre, other[None])[0]), sign, other))
    d_other, sign, other = min(out, key=lambda t: t[0])
    near = shortcut_bound(res)
    # own voxel: on the far side of the centre on `axis`, as far out as stays under the bound, nudged on the next axis so that its distance exceeds the other's where it can
    best = None
    ulp = float(np.spacing(np.abs(centre[axis])))
    n0 = int(math.sqrt(float(near)) / ulp)
    for n in range(n0 + 1, n0 - 3, -1):
        for mm in range(0, 12):
            own = centre.copy()
            own[axis] = f32(float(centre[axis]) - sign * n * ulp)
            b = (axis + 1) % 3
            own[b] = f32(float(centre[b]) + mm * float(np.spacing(np.abs(centre[b]))))
            d = float(sqdist(centre, own[None])[0])
            if d < float(near) and (best is None or d > best[0]):
                best = (d, own)
    return other, best[1]


def offset_pairs(n_pairs, offset, seed, seed_res=0.08, voxel_res=0.008):
    """n_pairs isolated pairs of seed cells, four cells apart, in a cube lattice that starts at `offset` metres on every axis.  Each pair: an own-cell voxel just inside
    the shortcut bound on one side of the centre, and a voxel just across the opposite face, level with the centre on the other two axes.  The axis of every pair is
    drawn from `seed`.  One point per voxel; no anchors (voxel borders do not matter: the points of a pair are ten voxels apart)."""
    rng = np.random.default_rng(seed)
    side = int(math.ceil(n_pairs ** (1.0 / 3.0)))
    sites = np.array([(i, j, k) for i in range(side) for j in range(side) for k in range(side)], np.int64)[:n_pairs]
    axes = rng.integers(0, 3, n_pairs)
    res = float(f32(seed_res))
    nominal = (offset + (sites * 4 + 2.5) * res).astype(f32)       # a voxel per pair, mid-cell, and the corner voxel the grid starts from
    corner = np.full((1, 3), offset, f32)
    draft = np.vstack([corner, nominal])
    g = grow_grid(draft, seed_res)
    pts = [corner[0]]
    for i in range(n_pairs):
        key = g.keys[1 + i]
        centre = ((key.astype(np.float64) + 0.5) * g.res + g.min).astype(f32)
        other, own = _axis_hit(g, key, centre, int(axes[i]))
        pts += [own, other]
    xyz = np.array(pts, f32)
    out = np.zeros((len(xyz), 4), f32)
    out[:, :3] = xyz
    out[:, 3] = np.uint32(V.GREY).view(f32)
    return np.ascontiguousarray(out)


# ------------------------------------------------------------------------------------------------ the cases
Case = collections.namedtuple("Case", "name family build params cond")
CASES = []


def case(name, family, build, cond, m=7, **params):
    p = dict(voxel_res=RD, seed_res=m * RD, use_transform=0)
    p.update(params)
    CASES.append(Case(name, family, build, p, cond))


def _line(xs):
    return lambda: V.cloud(np.array([(x, 0, 0) for x in xs], np.int64), RD, offset=0.25)


def _a5_every_direction():
    """The first voxel in leaf order alone in the lowest octant of the voxel cube, every extreme of the cloud in another octant: the second voxel lies below it on x and y and above on z, the third the other way round."""
    cells = np.array([(10, 10, 10), (0, 0, 20), (20, 20, 0), (23, 20, 20), (20, 23, 20), (20, 20, 23)], np.int64)
    off = np.array([(.5, .5, .5), (.25, .25, .5), (.5, .5, .25), (.75, .5, .5), (.5, .75, .5), (.5, .5, .75)])
    return V.cloud(cells, RD, offset=off, anchor=False)


def _a7_cube_edge():
    """Voxels 0..3 in the first cell, voxel 4 at q = 4 grows the cube to [-4, 12 - eps) on x, voxel 5 is the last float below 12: inside the cube of side 16, outside [min, max)."""
    pts = V.cloud(np.array([(x, 0, 0) for x in (0, 1, 2, 3, 4, 12)], np.int64), RD, offset=0.25)
    top = f32(12.25 * RD)
    assert pts[5, 0] == top
    pts[5, 0] = np.nextafter(top, f32(0))
    return pts


def _a8_block_and_outlier():
    """64 x 32 x 32 voxels inside the first cube and one voxel beyond it that is the last in leaf order: the upper corner of the cloud (it pins the voxel grid as the upper
    anchor would).  V = 65 537: its chunk is the 257th, which d_seed_grow's chunk search reaches on a thread's second trip."""
    cells = np.vstack([V.block(64, 32, 32), [[71, 31, 31]]])
    off = np.full((len(cells), 3), 0.5)
    off[0] = 0.25; off[-1] = 0.75
    return V.cloud(cells, RD, offset=off, anchor=False)


M = 7                     # seed_res / voxel_res of families B and C: r = 3.5 voxels, r2 = 12.25, floor(min_points) = 1
H = M / 2.0


def _centre(j):
    return (np.asarray(j, np.float64) + 0.5) * M


def _b1_shortcut_and_not():
    """Cell (2,0,0): a voxel at the centre (shortcut).  Cell (4,0,0): one voxel in a corner, 3 sqrt(3) from the centre, nothing around it (no shortcut, still its own).
    Cells (6,0,0) and (6,2,0): a voxel at 3.4375 and at 3 from the centre, under the bound of 3.4983."""
    return seed_frame(np.vstack([_centre((2, 0, 0)), _centre((4, 0, 0)) - 3.0, _centre((6, 0, 0)) + (3.4375, 0, 0), _centre((6, 2, 0)) + (3, 0, 0)]))


def _b2_corner_cut():
    """Cell (2,2,2) holds one voxel in its far corner; the voxel of cell (3,2,2) just across the face is nearer to its centre, and is its own cell's seed too (B7)."""
    return seed_frame(np.vstack([_centre((2, 2, 2)) - 3.0, _centre((2, 2, 2)) + (3.75, 0, 0)]))


def _b3_ties():
    """Inside a cell: voxels at +-1 from the centre on x, and the eight corners of a cube of side 1 around another centre.  Across two cells: an own voxel at (+-3, +-1.5, +-1)
    from the centre (3^2 + 1.5^2 + 1^2 = 3.5^2) and the voxel of the next cell at exactly 3.5 on x (it lies on the face, which belongs to the upper cell), in eight sign
    combinations so that the lower ordinal falls on either side; and an own voxel ON the lower face with its mirror image on the upper one."""
    q = [_centre((2, 0, 0)) + (1, 0, 0), _centre((2, 0, 0)) - (1, 0, 0)]
    q += list(_centre((4, 0, 0)) + grid3((-0.5, 0.5)))
    n = 0
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                j = (2 * (n % 4), 2 + 2 * (n // 4), 2)
                q += [_centre(j) + (3 * sx, 1.5 * sy, 1 * sz), _centre(j) + (H, 0, 0)]
                jz = (2 * (n % 4) + 10, 2 + 2 * (n // 4), 2)       # ... and with the other voxel on the z face: x decides the order of two voxels before z does
                q += [_centre(jz) + (3 * sx, 1.5 * sy, 1 * sz), _centre(jz) + (0, 0, H)]
                n += 1
    q += [_centre((2, 6, 2)) - (H, 0, 0), _centre((2, 6, 2)) + (H, 0, 0)]
    return seed_frame(np.array(q))


def _b5_cell_sizes():
    return seed_frame(np.vstack([cell_slots(M, (2 * i, 0, 0), n) for i, n in enumerate((1, 64, 65, 256, 257, 343), start=1)]))


def _b6_big_blocks():
    """Eight hollow cells side by side (no voxel nearer than 3.5 to its centre: no shortcut, 27-blocks of ~1300 voxels) and, apart, two hollow cells side by side (~320)."""
    q = [cell_slots(M, (i, j, k), hollow=3.6) for i in (1, 2) for j in (1, 2) for k in (1, 2)]
    q += [cell_slots(M, (5, 1, 1), hollow=3.6), cell_slots(M, (6, 1, 1), hollow=3.6)]
    return seed_frame(np.vstack(q))


def _c1_counts():
    """Isolated voxels at their cells' centres (num = 1 = floor(min_points): dropped), pairs one voxel apart (2: kept), a triple."""
    q = [_centre((2, 0, 0)), _centre((4, 0, 0)), _centre((4, 0, 0)) + (1, 0, 0), _centre((6, 0, 0)), _centre((6, 0, 0)) + (1, 0, 0), _centre((6, 0, 0)) - (1, 0, 0)]
    return seed_frame(np.array(q))


def _c2_at_the_radius():
    """A seed voxel at its cell's centre and a voxel at (3, 1.5, 1) from it: distance^2 = 12.25 = r2 exactly, not counted, so the seed is dropped; beside it the same
    with the second voxel at (3, 1.5, 0.9375): counted, kept."""
    q = [_centre((2, 0, 0)), _centre((2, 0, 0)) + (3, 1.5, 1), _centre((4, 0, 0)), _centre((4, 0, 0)) + (3, 1.5, 0.9375)]
    return seed_frame(np.array(q))


def _c3_eight_cells():
    """Eight voxels one voxel from the corner shared by the cells (2..3)^3, one in each: every seed counts all eight (distance^2 <= 12 < 12.25) in eight cells."""
    return seed_frame(grid3((3 * M - 1.0, 3 * M + 1.0)))


def _c4_own_cell_only():
    """A seed voxel at the centre of cell (2,2,2) with two voxels beside it; the six face neighbours hold a voxel each, 4 voxels from it: looked up, nothing counted."""
    c = _centre((2, 2, 2))
    q = [c, c + (1, 0, 0), c - (0, 1, 0)] + [c + 4.0 * np.eye(3)[a] * s for a in range(3) for s in (-1, 1)]
    return seed_frame(np.array(q))


def _c5_pruned_neighbours():
    """A solid block of 3 x 2 x 2 cells: every seed voxel lies by its cell's centre, so the sphere around it reaches at most eight cells and the occupied ones beyond are pruned."""
    return seed_frame(np.vstack([cell_slots(M, (i, j, k)) for i in (1, 2, 3) for j in (1, 2) for k in (1, 2)]))


def _c8_face_near_the_radius():
    """A seed voxel 3.375 from the lower face of its cell and a voxel 1/16 beyond that face, 3.4375 from it: counted, in a cell whose box is at 0.93 r2 -- inside the
    pruning margin by seven percent, outside it if the margin were 0.9."""
    c = _centre((3, 2, 2))
    return seed_frame(np.array([c + (-0.125, 0, 0), c + (-0.125 - 3.4375, 0, 0)]))


def _exact_min_points(target=2.0):
    """A float32 seed_res near 7.14 / 64 whose min_points (the float32 expression) is exactly `target`: num = 2 is then NOT more than min_points."""
    s = f32(math.sqrt(target / (0.05 * math.pi)) * 2 * RD)
    lo = s
    for _ in range(4096):
        lo = np.nextafter(lo, f32(0))
    x = lo
    for _ in range(8192):
        if min_points(x, RD) == f32(target):
            return float(x)
        x = np.nextafter(x, f32(1))
    return None


EXACT_SEED_RES = _exact_min_points()


def _c9_pairs():
    return seed_frame(np.array([(20, 0, 0), (21, 0, 0), (40, 0, 0), (41, 0, 0), (41, 1, 0), (60, 0, 0)], np.float64))


# A. growth
case("a1-single-cell", "A", lambda: V.cloud(V.block(3, 3, 3), RD), ("events", 1, 1), m=8)
case("a2-triggers-at-0-255-256", "A", _line(list(range(255)) + [256, 768]), ("triggers", (0, 255, 256)), m=256)
case("a3-two-events-in-a-chunk", "A", _line([0, 1, 2, 3, 4, 12]), ("triggers", (0, 4, 5)), m=4)
case("a4-event-at-the-last-voxel", "A", _line([0, 1, 2]), ("last_voxel",), m=3)
case("a5-every-direction", "A", _a5_every_direction, ("directions",), m=2)
case("a6-thirteen-events", "A", _line([0] + [2 * (2 ** k - 1) for k in range(1, 13)]), ("events", 12, 48), m=2)
case("a7-cube-edge", "A", _a7_cube_edge, ("edge",), m=4)
case("a8-second-chunk-trip", "A", _a8_block_and_outlier, ("second_trip", 65537), m=64)
case("a9-thirteen-events-desc", "A", _line([0] + [2 * (2 ** k - 1) for k in range(1, 13)]), ("lower_events", 12), m=2, leaf_order=1)
# B. nearest voxel
case("b1-shortcut-and-not", "B", _b1_shortcut_and_not, ("b1",))
case("b2-b7-corner-cut", "B", _b2_corner_cut, ("other_cell",))
case("b3-ties", "B", _b3_ties, ("ties",))
case("b4-key-zero", "B", lambda: V.cloud(V.block(12, 12, 12), RD), ("key_zero",), m=4, leaf_order=1)
case("b5-cell-sizes", "B", _b5_cell_sizes, ("cell_sizes", (1, 64, 65, 256, 257, 343)))
case("b6-big-blocks", "B", _b6_big_blocks, ("big_blocks",))
# C. filter
case("c1-counts", "C", _c1_counts, ("counts",))
case("c2-at-the-radius", "C", _c2_at_the_radius, ("at_r2",))
case("c3-eight-cells", "C", _c3_eight_cells, ("eight_cells",))
case("c4-own-cell-only", "C", _c4_own_cell_only, ("own_only",))
case("c5-pruned-neighbours", "C", _c5_pruned_neighbours, ("pruned",))
case("c6-every-seed-dropped", "C", lambda: seed_frame(V.lattice(6, 14).astype(np.float64)), ("all_dropped", 200))
case("c7-every-seed-kept", "C", lambda: V.cloud(V.block(20, 20, 2), RD, rgba="random"), ("all_kept", 16), m=5)
case("c8-face-near-the-radius", "C", _c8_face_near_the_radius, ("prune_slack", 0.9, 1.0))
case("c9-min-points-exactly-2", "C", _c9_pairs, ("exact_min_points", 2), seed_res=EXACT_SEED_RES)
# D. large offsets
D_PAIRS = 600
D_SEED = 1
case("d-offset-600", "D", lambda: offset_pairs(D_PAIRS, 600.0, D_SEED), ("shortcut_unsound", 3), voxel_res=0.008, seed_res=0.08)
case("d-offset-0", "D", lambda: offset_pairs(D_PAIRS, 0.0, D_SEED), ("shortcut_sound",), voxel_res=0.008, seed_res=0.08)

CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)
NAMES = [c.name for c in CASES]
BATCH = ["b1-shortcut-and-not", "b5-cell-sizes", "b6-big-blocks", "c6-every-seed-dropped"]      # family E: one batch, one set of parameters, 5 to 217 cells
NARROW = ["a2-triggers-at-0-255-256", "b5-cell-sizes", "c1-counts"]


@functools.lru_cache(maxsize=None)
def frame_of(name):
    pts = CASE[name].build()
    pts.setflags(write=False)
    return pts


def params_of(P, name):
    return P.launch_params(**CASE[name].params)


Run = collections.namedtuple("Run", "case pts prm labels res h census seconds")
_runs = {}


def oracle_run(oracle, P, name):
    """The oracle's run of a case, the reference of its voxel centroids and the census, made once per process and shared (read-only)."""
    if name not in _runs:
        import time
        pts, prm = frame_of(name), params_of(P, name)
        t0 = time.perf_counter()
        rc, labels, res, h = oracle.segment(pts, prm)
        dt = time.perf_counter() - t0
        assert rc == 0, "the oracle refuses case %s: %d" % (name, rc)
        xyz = h.get("VOXEL_XYZ").reshape(-1, 3)
        _runs[name] = Run(CASE[name], pts, prm, labels, res, h, census(xyz, prm.seed_res, prm.voxel_res), dt)
    return _runs[name]


def equals(name, a, b):
    return first_mismatch(name, np.ascontiguousarray(a), np.ascontiguousarray(b))


# ------------------------------------------------------------------------------------------------ the conditions
def check_condition(r):
    """Assert that the census of a case (from the brute-force reference of the oracle's voxel centroids) meets the condition that makes the case reach its branch."""
    cen, cells = r.census, r.census.cells
    what, args = r.case.cond[0], r.case.cond[1:]
    ev = cen.events
    assert (cen.V <= 20000 or what == "second_trip") and len(ev) <= MAX_SEED_EVENTS
    if what == "events":
        assert args[0] <= len(ev) <= args[1], len(ev)
        if args == (1, 1):
            assert cen.C == 1
    elif what == "triggers":
        assert tuple(e.trigger for e in ev) == args[0], [e.trigger for e in ev]
        if 255 in args[0]:
            assert cen.chunk_pos == [0, 255, 0]
        else:
            assert len({e.trigger // SEED_CHUNK for e in ev[1:]}) == 1 and len(ev) >= 3
    elif what == "last_voxel":
        assert ev[-1].trigger == cen.V - 1 and len(ev) >= 2
    elif what == "directions":
        assert all(any(e.lower[a] for e in ev) and any(e.upper[a] for e in ev) for a in range(3)), ev
    elif what == "edge":
        assert any(e.edge for e in ev), ev
    elif what == "second_trip":
        assert cen.V == args[0] and all(e.trigger < SEED_CHUNK for e in ev[:-1]) and ev[-1].trigger >= 256 * SEED_CHUNK and len(ev) >= 2, [e.trigger for e in ev]
    elif what == "lower_events":
        assert len(ev) >= args[0] and all(any(e.lower) for e in ev[1:]) and r.prm.leaf_order == 1
    elif what == "b1":
        short = [c for c in cells if c.shortcut]
        plain = [c for c in cells if not c.shortcut and not c.other_cell]
        assert short and plain and any(c.own_min == 0 for c in short), (len(short), len(plain))
    elif what == "other_cell":
        other = [i for i, c in enumerate(cells) if c.other_cell and not c.shortcut]
        assert other and len(set(cen.ref.seed_orig.tolist())) < cen.C, other          # B7: one voxel is the nearest of two cells
    elif what == "ties":
        inside = [c for c in cells if c.tied and len(c.tie_cells) == 1]
        across = [c for c in cells if c.tied and len(c.tie_cells) == 2 and not c.shortcut]
        assert len(inside) >= 2 and sum(c.tie_winner_other for c in across) >= 1 and sum(not c.tie_winner_other for c in across) >= 1, (len(inside), [c.tie_winner_other for c in across])
        assert any(c.own_min == f32(0.25 * cen.ref.grid.res ** 2) for c in across)      # an own voxel at exactly half a cell: under the bound only if the margin had the wrong sign
    elif what == "key_zero":
        zeros = {int((k == 0).sum()) for k in cen.ref.cell_keys}
        assert {1, 2, 3} <= zeros, zeros
    elif what == "cell_sizes":
        have = {c.n_own for c in cells}
        assert set(args[0]) <= have, sorted(have)
    elif what == "big_blocks":
        slow = [c.n_block for c in cells if not c.shortcut]
        assert any(CAND_STRIDE < n <= 2 * CAND_STRIDE for n in slow) and any(n > 2 * CAND_STRIDE for n in slow), sorted(slow)
    elif what == "counts":
        assert any(c.margin == 0 for c in cells) and any(c.margin == 1 for c in cells) and any(c.margin == 2 for c in cells), [c.margin for c in cells]
        assert set(cen.ref.keep.tolist()) == {True, False}
    elif what == "at_r2":
        at = [i for i, c in enumerate(cells) if c.at_r2 and c.margin == 0]
        assert at and not cen.ref.keep[at].any() and cen.ref.keep.any(), at
    elif what == "eight_cells":
        assert sum(c.counted_cells == 8 for c in cells) == 8, [c.counted_cells for c in cells]
    elif what == "own_only":
        mid = [c for c in cells if c.own_min == 0 and c.counted_cells == 1 and c.margin >= 1 and c.n_block > c.n_own and c.kept_cells == 7]
        assert mid, [(c.own_min, c.counted_cells, c.margin, c.kept_cells) for c in cells]
    elif what == "pruned":
        assert sum(c.pruned_occupied > 0 for c in cells) >= 8 and all(c.kept_cells <= 8 for c in cells), [(c.pruned_occupied, c.kept_cells) for c in cells]
    elif what == "all_dropped":
        assert cen.C >= args[0] and not cen.ref.keep.any() and r.res.n_seeds == 0
    elif what == "all_kept":
        assert cen.C >= args[0] and cen.ref.keep.all()
    elif what == "prune_slack":
        assert any(args[0] < c.prune_slack < args[1] and c.margin == 1 and c.counted_cells == 2 for c in cells), [c.prune_slack for c in cells]      # ... and that voxel decides whether the seed is kept
    elif what == "exact_min_points":
        assert cen.ref.min_points == f32(args[0]) and any(c.margin == 0 and cen.ref.num[i] == args[0] for i, c in enumerate(cells)) and any(c.margin == 1 for c in cells)
    elif what == "shortcut_unsound":
        bad = [i for i, c in enumerate(cells) if c.shortcut and c.other_cell]
        assert len(bad) >= args[0], len(bad)
    elif what == "shortcut_sound":
        assert not [i for i, c in enumerate(cells) if c.shortcut and c.other_cell] and sum(c.shortcut for c in cells) >= D_PAIRS // 2
    else:
        raise AssertionError("unknown condition %r" % (what,))
