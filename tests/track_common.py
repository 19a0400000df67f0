"""Shared by tests/test_track_cpu.py and tests/test_track_gpu.py: the numpy reference of a tracker update (include/f3ds.h, "label tracker", steps 1-6) in
float32 arithmetic in the stated operation order on top of rgbd_common.numpy_deproject, its assignment a plain Python loop; and the generators of the
frames both files run: blocky label images over depth planes and steps, holes, seeded poses.

The reference counts how often each branch of the definition was taken (RefTracker.counters), so that a test can assert that its inputs reached it."""
import numpy as np

from rgbd_common import SIZES, frame_format, numpy_deproject

NO = 0xFFFFFFFF
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -7
FORMATS = SIZES + [(97, 61)]
RESULT_FIELDS = ("n_regions", "n_nonempty", "n_matched", "n_new", "n_retired", "n_entries", "next_id", "first_frame", "n_labelled", "n_votes")
BRANCHES = ("tie", "permille", "min_votes", "slot_claimed", "region_assigned", "depth", "outside", "retired")
f32 = np.float32


# ---- steps 2 and 3 -------------------------------------------------------------------------------------------------------------------------------------
def numpy_reproject(fmt, pts, pose):
    """(pixel index in the previous frame or -1 (int32), zp (float32)) of (N, 4) float32 records; pose: None or 12 floats, row-major 3 x 4."""
    x, y, z = pts[:, 0].astype(f32), pts[:, 1].astype(f32), pts[:, 2].astype(f32)
    w, h = int(fmt.width), int(fmt.height)
    fx, fy, cx, cy = f32(fmt.fx), f32(fmt.fy), f32(fmt.cx), f32(fmt.cy)
    with np.errstate(all="ignore"):
        if pose is None:
            xp, yp, zp = x, y, z
        else:
            r = np.asarray(pose, f32).reshape(12)
            xp = ((r[0] * x + r[1] * y) + r[2] * z) + r[3]
            yp = ((r[4] * x + r[5] * y) + r[6] * z) + r[7]
            zp = ((r[8] * x + r[9] * y) + r[10] * z) + r[11]
        uf = (xp * fx) / zp + cx
        vf = (yp * fy) / zp + cy
        us, vs = uf + f32(0.5), vf + f32(0.5)
        assert us.dtype == f32 and vs.dtype == f32 and zp.dtype == f32
        ok = (zp > 0) & np.isfinite(zp) & (us >= 0) & (us < f32(w)) & (vs >= 0) & (vs < f32(h))
        ui = np.floor(np.where(ok, us, f32(0))).astype(np.int64)
        vi = np.floor(np.where(ok, vs, f32(0))).astype(np.int64)
    return np.where(ok, vi * w + ui, -1).astype(np.int32), zp


# ---- step 5 --------------------------------------------------------------------------------------------------------------------------------------------
def ref_assign(min_votes, min_permille, size, entries, prev_id, next_id, counters=None):
    """(rc, ids, next_id, result dict).  entries: rows (i, j, c).  Plain Python integers throughout."""
    cnt = counters if counters is not None else {}
    size = [int(s) for s in size]
    prev_id = [int(p) for p in prev_id]
    el = []
    for i, j, c in ((int(a), int(b), int(c)) for a, b, c in entries):
        if c < max(int(min_votes), 1):
            cnt["min_votes"] = cnt.get("min_votes", 0) + 1
        elif c * 1000 < int(min_permille) * size[i]:
            cnt["permille"] = cnt.get("permille", 0) + 1
        else:
            el.append((c, i, j))
    el.sort(key=lambda e: (-e[0], e[1], e[2]))
    if any(a[0] == b[0] for a, b in zip(el, el[1:])):
        cnt["tie"] = cnt.get("tie", 0) + 1
    ids = [NO] * len(size)
    claimed = set()
    matched = 0
    for c, i, j in el:
        if ids[i] != NO:
            cnt["region_assigned"] = cnt.get("region_assigned", 0) + 1
        elif j in claimed:
            cnt["slot_claimed"] = cnt.get("slot_claimed", 0) + 1
        else:
            ids[i] = prev_id[j]; claimed.add(j); matched += 1
    new = [i for i in range(len(size)) if size[i] > 0 and ids[i] == NO]
    if int(next_id) + len(new) >= 0xFFFFFFFF:
        return ERR_UNSUPPORTED, None, int(next_id), None
    nxt = int(next_id)
    for i in new:
        ids[i] = nxt; nxt += 1
    retired = sum(1 for j, p in enumerate(prev_id) if p != NO and j not in claimed)
    if retired:
        cnt["retired"] = cnt.get("retired", 0) + 1
    res = dict(n_regions=len(size), n_nonempty=sum(1 for s in size if s > 0), n_matched=matched, n_new=len(new), n_retired=retired, n_entries=len(entries),
               next_id=nxt, first_frame=0, n_labelled=sum(size), n_votes=sum(int(e[2]) for e in entries))
    return OK, np.array(ids, np.uint32), nxt, res


# ---- the whole update ------------------------------------------------------------------------------------------------------------------------------------
class RefTracker:
    def __init__(self, min_votes=16, min_permille=300, depth_tol=0.05):
        self.min_votes, self.min_permille, self.depth_tol = int(min_votes), int(min_permille), f32(depth_tol)
        self.next_id = 0
        self.counters = {}
        self.reset()
        self.ids = None

    def reset(self):
        self.slot = self.z = self.fmt_key = None
        self.prev_id = np.zeros(0, np.uint32)

    def votes(self, fmt, depth, labels, n_regions, pose):
        """(rc, labelled mask, size, entries (i, j, c) in (i, j) order, z per pixel) of steps 1-4"""
        h, w = int(fmt.height), int(fmt.width)
        labels = np.asarray(labels, np.uint32).reshape(-1)
        pts = numpy_deproject(fmt, depth, np.zeros((h, w), np.uint32))
        z = pts[:, 2]
        valid = ~np.isnan(z)
        if ((labels != NO) & (labels >= n_regions)).any():
            return ERR_ARG, None, None, None, None
        labelled = valid & (labels != NO)
        size = np.bincount(labels[labelled], minlength=n_regions).astype(np.int64)
        entries = np.zeros((0, 3), np.int64)
        if self.slot is not None:
            pixel, zp = numpy_reproject(fmt, pts, pose)
            landed = labelled & (pixel >= 0)
            self.counters["outside"] = self.counters.get("outside", 0) + int((labelled & (pixel < 0)).sum())
            q = np.where(landed, pixel, 0)
            j = self.slot[q]
            with np.errstate(all="ignore"):
                near = np.abs(zp - self.z[q]) <= self.depth_tol * zp
            self.counters["depth"] = self.counters.get("depth", 0) + int((landed & (j != NO) & ~near).sum())
            vote = landed & (j != NO) & near
            if vote.any():
                pairs = np.stack([labels[vote].astype(np.int64), j[vote].astype(np.int64)], axis=1)
                uniq, c = np.unique(pairs, axis=0, return_counts=True)
                entries = np.concatenate([uniq, c[:, None]], axis=1)
        return OK, labelled, size, entries, z

    def update(self, fmt, depth, labels, n_regions, pose=None):
        """(rc, track id per pixel, id per region, result dict); the state changes only when rc == 0"""
        key = (int(fmt.width), int(fmt.height), f32(fmt.fx), f32(fmt.fy), f32(fmt.cx), f32(fmt.cy))
        if self.fmt_key is not None and key != self.fmt_key:
            return ERR_ARG, None, None, None
        labels = np.asarray(labels, np.uint32).reshape(-1)
        rc, labelled, size, entries, z = self.votes(fmt, depth, labels, n_regions, pose)
        if rc:
            return rc, None, None, None
        rc, ids, nxt, res = ref_assign(self.min_votes, self.min_permille, size, entries, self.prev_id, self.next_id, self.counters)
        if rc:
            return rc, None, None, None
        res["first_frame"] = 1 if self.slot is None else 0
        out = np.full(len(labels), NO, np.uint32)
        has = labels != NO
        out[has] = ids[labels[has]]
        self.slot = np.where(labelled, labels, np.uint32(NO)).astype(np.uint32)
        self.z = np.where(np.isnan(z), f32(np.nan), z).astype(f32)
        self.prev_id, self.next_id, self.fmt_key, self.ids = ids, nxt, key, ids
        return OK, out, ids, res


# ---- generators ----------------------------------------------------------------------------------------------------------------------------------------
def track_format(P, width, height, depth="u16"):
    return frame_format(P, width, height, depth, "rgb8", 0.001 if depth == "u16" else 0.00125)


def to_depth(mm, depth_kind):
    """millimetres (float array, 0 = no measurement) as the depth image of track_format: u16 millimetres, or f32 units of 1.25 mm"""
    mm = np.asarray(mm, np.float64)
    if depth_kind == "u16":
        return np.rint(mm).astype(np.uint16)
    return (np.rint(mm).astype(f32) * f32(0.8)).astype(f32)


def blocks(width, height, nx, ny):
    """a label image of nx * ny rectangular blocks, labels in row-major block order"""
    u = np.minimum(np.arange(width) * nx // width, nx - 1)
    v = np.minimum(np.arange(height) * ny // height, ny - 1)
    return (v[:, None] * nx + u[None, :]).astype(np.uint32)


def seeded_pose(rng, max_deg=5.0, max_t=0.2):
    """a rotation of up to max_deg degrees about a random axis and a translation of up to max_t metres per axis, as 12 float32"""
    axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
    a = np.deg2rad(rng.uniform(-max_deg, max_deg))
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    t = rng.uniform(-max_t, max_t, 3)
    return np.concatenate([R, t[:, None]], axis=1).astype(f32).reshape(12)


def column_shift_pose(fmt, z_m, k):
    """the pose under which a plane at depth z_m (metres, as float32 arithmetic sees it) moves k columns to the right: t0 = k * z / fx"""
    pose = np.eye(3, 4, dtype=f32).reshape(12)
    pose[3] = f32(k) * f32(z_m) / f32(fmt.fx)
    return pose


def random_scene(rng, width, height, n_regions, depth_kind, holes=0.10, unlabelled=0.05):
    """(depth image, label image (h, w) uint32): rectangles painted over each other (a label may vanish under later ones: an empty region), every
    region a plane with a depth step to its neighbours and a small slope; 10 % of the pixels without a measurement, 5 % without a label"""
    lab = np.zeros((height, width), np.uint32)
    mm = np.zeros((height, width), np.float64)
    uu, vv = np.meshgrid(np.arange(width), np.arange(height))
    for r in range(n_regions):
        if r == 0:
            u0, v0, u1, v1 = 0, 0, width, height
        else:
            u0, v0 = int(rng.integers(0, width)), int(rng.integers(0, height))
            u1, v1 = u0 + int(rng.integers(1, max(2, width // 2))), v0 + int(rng.integers(1, max(2, height // 2)))
        base, su, sv = rng.uniform(800, 3000), rng.uniform(-2, 2), rng.uniform(-2, 2)
        lab[v0:v1, u0:u1] = r
        mm[v0:v1, u0:u1] = (base + su * uu + sv * vv)[v0:v1, u0:u1]
    mm = np.clip(mm, 300, 60000)
    mm[rng.random((height, width)) < holes] = 0
    lab[rng.random((height, width)) < unlabelled] = NO
    return to_depth(mm, depth_kind), lab


def random_sequence(P, seed, n_frames=3):
    """A seeded sequence of frames of one camera: dict(fmt, depth_kind, params, frames = [dict(depth, labels, n_regions, pose)]).  Every frame after the
    first repaints a few rectangles of the one before (regions split, merge, appear and vanish), renumbers the labels and moves the camera by a seeded
    pose whose size varies from nothing to 5 degrees / 0.2 m."""
    rng = np.random.default_rng(1000 + seed)
    width, height = [(67, 45), (97, 61), (40, 30)][seed % 3]
    depth_kind = "u16" if seed % 2 == 0 else "f32"
    fmt = track_format(P, width, height, depth_kind)
    K = int(rng.integers(1, 41))
    params = dict(min_votes=int(rng.choice([0, 1, 4, 16])), min_permille=int(rng.choice([0, 100, 300, 600])), depth_tol=float(rng.choice([0.01, 0.05, 0.2])))
    depth, lab = random_scene(rng, width, height, K, depth_kind)
    frames = [dict(depth=depth, labels=lab, n_regions=K, pose=None)]
    mm_scale = 1.0 if depth_kind == "u16" else 0.8
    for _ in range(1, n_frames):
        depth, lab = depth.copy(), lab.copy()
        for _ in range(int(rng.integers(0, 4))):      # repaint: a new or an existing label over a rectangle, on its own plane or on the old depths
            u0, v0 = int(rng.integers(0, width)), int(rng.integers(0, height))
            u1, v1 = u0 + int(rng.integers(1, width // 2)), v0 + int(rng.integers(1, height // 2))
            if rng.random() < 0.5:
                lab[v0:v1, u0:u1] = K; K += 1
            else:
                lab[v0:v1, u0:u1] = int(rng.integers(0, K))
            if rng.random() < 0.5:
                depth[v0:v1, u0:u1] = np.asarray(rng.uniform(800, 3000) * mm_scale).astype(depth.dtype)
        perm = rng.permutation(K).astype(np.uint32)
        has = lab != NO
        lab[has] = perm[lab[has]]
        flip = rng.random((height, width)) < 0.03      # holes come and go
        depth[flip] = 0
        scale = float(rng.choice([0.0, 0.05, 1.0]))
        pose = None if scale == 0.0 else seeded_pose(rng, 5.0 * scale, 0.2 * scale)
        frames.append(dict(depth=depth, labels=lab, n_regions=K, pose=pose))
    return dict(fmt=fmt, depth_kind=depth_kind, params=params, frames=frames)


RANDOM_SEEDS = list(range(24))


def run_reference(seq):
    """the reference over a sequence: (list of (rc, ids image, ids, result), counters)"""
    ref = RefTracker(**seq["params"])
    out = [ref.update(seq["fmt"], f["depth"], f["labels"], f["n_regions"], f["pose"]) for f in seq["frames"]]
    return out, ref.counters
