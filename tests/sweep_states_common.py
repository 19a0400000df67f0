"""Hand-built start-of-run states for the label-propagation sweeps (d_sweep_begin .. d_centroid), a literal reference of expandSupervoxels that runs from them, and
the cases (tests/test_sweep_states_cpu.py, tests/test_sweep_states_gpu.py).

Three parties.  The kernel probe (tests/kernprobe: kp_sweeps) runs the product's sweep kernels from a State; the CPU emulation (tests/emul: f3ds_emul_sweeps_from) walks
the device's reformulation -- sweep control, R rounds, thief masks, walkers -- from the same State and takes the census; expand() below restates the oracle's
expand_loop (oracle/f3ds_oracle.cpp) in plain Python: a sorted leaf set per helper, an owner and a distance per voxel, helpers in label order, the strict <, the loser's
leaf erased at once, the winner's leaves added after its turn, empty helpers erased, updateCentroid.  It takes nothing from the oracle library and nothing from the
emulation; the feature distance is n_voxel_distance (csrc/f3ds_numerics.h) operation by operation in numpy float32.  A ghost leaf is a member of a helper's set whose
owner is somebody else.

The lattice: integer cells, voxels in Morton order of the cells (x the highest bit of a triple, as the product orders its leaves), so the 64- and 128-voxel tiles are
the product's; neighbour slot = (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1); positions are cell centres on the pitch 2^-6, so every spatial distance is a dyadic rational.

Every case carries the condition its census has to meet (cond(run) -> None or what is wrong), in the style of vccs_clouds_common.CASES."""
import numpy as np

import kernprobe_inputs as K
from vccs_clouds_common import BY_WAVE_RATIO, HT_CAP, HT_ROW, NT_TILE, QL, R_ROUNDS, R_STACK  # noqa: F401  (the constants the cases are sized by)

F = np.float32
U32 = np.uint32
FLT_MAX = F(3.402823466e+38)
PITCH = 2.0 ** -6
BOOKS = ("row", "wave", "raw_overflow", "window", "max_gain", "max_raw", "max_tiles", "tail")      # f3ds_emul_sweeps_from: books[8] per sweep
FULL, INCREMENTAL, FALLBACK, IDLE = 0, 1, 2, 3                                                     # sweep_stats


# ------------------------------------------------------------------------------------------------ lattice
def morton(cells):
    c = np.asarray(cells, np.int64)
    code = np.zeros(len(c), np.int64)
    for b in range(20, -1, -1):
        code = (code << 3) | (((c[:, 0] >> b) & 1) << 2) | (((c[:, 1] >> b) & 1) << 1) | ((c[:, 2] >> b) & 1)
    return code


class Lattice:
    def __init__(self, cells):
        cells = np.unique(np.asarray(cells, np.int64).reshape(-1, 3), axis=0)
        assert cells.min() >= 0
        self.cells = cells[np.argsort(morton(cells), kind="stable")]
        self.V = V = len(self.cells)
        key = lambda c: (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
        keys = key(self.cells)
        order = np.argsort(keys); skeys = keys[order]
        self.nbr = np.full((V, 27), -1, np.int32)
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    q = self.cells + (dx, dy, dz)
                    ok = (q >= 0).all(axis=1)
                    k = key(np.maximum(q, 0))
                    pos = np.minimum(np.searchsorted(skeys, k), V - 1)
                    hit = ok & (skeys[pos] == k)
                    self.nbr[hit, (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)] = order[pos[hit]]
        self.xyz = ((self.cells + 0.5) * PITCH).astype(F)

    def at(self, x, y, z):
        """ordinal of a cell"""
        i = np.flatnonzero((self.cells == (x, y, z)).all(axis=1))
        return int(i[0])


def corridor(n):
    return Lattice([(0, 0, z) for z in range(n)])          # (Morton order of (0, 0, z) is z: ordinal = position)


def block_cells(nx, ny, nz):
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1)


def near_cube(V):
    m = 1
    while m ** 3 < V:
        m += 1
    return Lattice(block_cells(m, m, m)[:V])


def features(lat, rng=None, rgb=(120, 130, 110), normal=(0.0, 0.0, 1.0)):
    vf = np.zeros((lat.V, 12), F)
    vf[:, 0:3] = lat.xyz
    if rng is None:
        vf[:, 3:6] = rgb; vf[:, 6:9] = normal
    else:
        vf[:, 3:6] = rng.integers(0, 256, (lat.V, 3))
        n = rng.normal(size=(lat.V, 3)).astype(F)
        vf[:, 6:9] = n / np.sqrt((n * n).sum(axis=1, dtype=F), dtype=F)[:, None]
    return vf


# ------------------------------------------------------------------------------------------------ the state
class State:
    """A start-of-run state in the convention d_helper_init and d_centroid leave (kp_sweeps' contract): hcount = owned voxels + the ghost leaf, hlo / hhi their lowest
    and highest ordinal (0, 0 without leaves), tl the tiles that hold an owned voxel, ascending (tcnt = HT_CAP + 1 when there are more than HT_CAP)."""

    def __init__(self, lat, vf, S0, owner, dist, hc, ghosts=None, seed_res=8 * PITCH, w_normal=1.0, w_color=1.0, w_spatial=1.0):
        self.V, self.S0, self.nbr = lat.V, S0, lat.nbr.copy()
        L = S0 + 1
        self.vf = np.ascontiguousarray(vf, F)
        self.owner = np.ascontiguousarray(owner, U32)
        self.dist = np.where(self.owner == 0, FLT_MAX, np.asarray(dist, F)).astype(F)
        self.hc = np.zeros((L, 12), F); self.hc[:, :9] = np.asarray(hc, F)[:, :9]
        self.ghost_vox = np.full(L, -1, np.int32); self.ghost_active = np.zeros(L, np.uint8)
        for h, v in (ghosts or {}).items():
            self.ghost_vox[h] = v; self.ghost_active[h] = 1
        self.seed_res, self.w_normal, self.w_color, self.w_spatial = float(seed_res), float(w_normal), float(w_color), float(w_spatial)
        self.books()

    def books(self):
        L = self.S0 + 1
        self.hcount = np.zeros(L, U32); self.hlo = np.zeros(L, U32); self.hhi = np.zeros(L, U32)
        self.tl = np.zeros((L, HT_CAP), U32); self.tcnt = np.zeros(L, U32)
        for h in range(1, L):
            own = np.flatnonzero(self.owner == h)
            leaves = np.union1d(own, [self.ghost_vox[h]] if self.ghost_active[h] else []).astype(np.int64)
            self.hcount[h] = len(leaves)
            if len(leaves):
                self.hlo[h], self.hhi[h] = leaves.min(), leaves.max()
            tiles = np.unique(own >> 6)
            self.tcnt[h] = len(tiles) if len(tiles) <= HT_CAP else HT_CAP + 1
            self.tl[h, :min(len(tiles), HT_CAP)] = tiles[:HT_CAP]

    def copy(self):
        o = State.__new__(State)
        for k, v in self.__dict__.items():
            o.__dict__[k] = v.copy() if isinstance(v, np.ndarray) else v
        return o


# ------------------------------------------------------------------------------------------------ the literal reference
def voxel_distance(c, v, seed_res, w_normal, w_color, w_spatial):
    """n_voxel_distance (csrc/f3ds_numerics.h) of one centroid row c against the rows v[n x 12], operation by operation in float32"""
    c = np.asarray(c, F); v = np.asarray(v, F).reshape(-1, 12)
    dx, dy, dz = c[0] - v[:, 0], c[1] - v[:, 1], c[2] - v[:, 2]
    spatial = np.sqrt(dx * dx + (dy * dy + dz * dz), dtype=F) / F(seed_res)          # n_sum3(a, b, c) = a + (b + c)
    er, eg, eb = c[3] - v[:, 3], c[4] - v[:, 4], c[5] - v[:, 5]
    color = np.sqrt(er * er + (eg * eg + eb * eb), dtype=F) / F(255.0)
    dot = (c[6] * v[:, 6] + c[7] * v[:, 7]) + (c[8] * v[:, 8] + F(0.0) * F(0.0))
    cosn = F(1.0) - np.abs(dot)
    out = (cosn * F(w_normal) + color * F(w_color)) + spatial * F(w_spatial)
    assert out.dtype == F
    return out


def expand(st, n):
    """n iterations of expand_loop from st.  Returns the per-sweep snapshots kp_sweeps returns (hc rows of erased helpers keep what they last held: compare the rows of
    helpers with hcount > 0 only) and `ties`: how often a helper's distance to a voxel of another helper equalled that voxel's distance bit for bit (no theft)."""
    V, S0 = st.V, st.S0
    L = S0 + 1
    owner = st.owner.astype(np.int64).copy(); dist = st.dist.copy(); hc = st.hc.copy()
    leaves = [None] * L
    for h in range(1, L):
        own = np.flatnonzero(owner == h)
        leaves[h] = set(own.tolist()) | ({int(st.ghost_vox[h])} if st.ghost_active[h] else set())
    alive = [h for h in range(1, L)]           # the helper list; a helper without leaves is erased after the sweep it is found empty in (start state included)
    out = dict(owner=np.zeros((n, V), U32), dist=np.zeros((n, V), F), hc=np.zeros((n, L, 12), F), hcount=np.zeros((n, L), U32), ghost_active=np.zeros((n, L), np.uint8),
               ghost_done=np.zeros((n, L), np.uint8), tcnt=np.zeros((n, L), U32), n_changed=np.zeros(n, U32))
    ties = 0
    prm = (st.seed_res, st.w_normal, st.w_color, st.w_spatial)
    with np.errstate(all="ignore"):
        for t in range(n):
            owner0 = owner.copy(); dist0 = dist.copy()
            for h in alive:                                          # SupervoxelHelper::expand
                if not leaves[h]:
                    continue
                lv = np.fromiter(sorted(leaves[h]), np.int64, len(leaves[h]))
                # leaf by leaf, neighbour slot by slot, a voxel is offered once: whatever the first offer decides, the later ones decide alike (stolen: it is h's now
                # and skipped; not stolen: same distance against the same d)
                cand = st.nbr[lv].reshape(-1)
                cand = cand[cand >= 0]
                _, first = np.unique(cand, return_index=True)
                cand = cand[np.sort(first)]
                cand = cand[owner[cand] != h]
                if not len(cand):
                    continue
                d = voxel_distance(hc[h], st.vf[cand], *prm)
                ties += int(((d.view(U32) == dist[cand].view(U32)) & (owner[cand] != 0)).sum())
                win = d < dist[cand]
                for v, dv in zip(cand[win].tolist(), d[win]):
                    dist[v] = dv
                    if owner[v]:
                        leaves[owner[v]].discard(v)
                    owner[v] = h
                leaves[h].update(cand[win].tolist())                 # new_owned, after the loop over the leaves
            for h in alive:                                          # erase the empty helpers, updateCentroid of the others
                if leaves[h]:
                    lv = np.fromiter(sorted(leaves[h]), np.int64, len(leaves[h]))
                    s = np.cumsum(st.vf[lv, 0:9], axis=0, dtype=F)[-1]      # float32, one leaf after the other in leaf order
                    hc[h] = K.centroid_finish(s, len(lv))
            alive = [h for h in alive if leaves[h]]
            o = out
            o["owner"][t] = owner; o["dist"][t] = dist; o["hc"][t] = hc
            for h in range(1, L):
                o["hcount"][t, h] = len(leaves[h])
                own = np.flatnonzero(owner == h)
                o["ghost_active"][t, h] = len(leaves[h]) > len(own)
                nt = len(np.unique(own >> 6))
                o["tcnt"][t, h] = nt if nt <= HT_CAP else HT_CAP + 1
            o["n_changed"][t] = int(((owner != owner0) | (dist.view(U32) != dist0.view(U32))).sum())
    out["ties"] = ties
    return out


# ------------------------------------------------------------------------------------------------ the emulation from a state
class EmulRun:
    pass


def emul_from(emul, st, n, inc_shift=6, r_rounds=R_ROUNDS):
    """f3ds_emul_sweeps_from: the snapshots and the census (sweep_stats, r_deep, r_deep_cold, rounds[n], books[n] as dicts of BOOKS)"""
    import ctypes
    V, L = st.V, st.S0 + 1
    c = lambda a, dt: np.ascontiguousarray(a, dt)
    ins = [c(st.nbr, np.int32), c(st.vf, F), c(st.owner, U32), c(st.dist, F), c(st.hc, F), c(st.hcount, U32), c(st.hlo, U32), c(st.hhi, U32), c(st.tl, U32), c(st.tcnt, U32),
           c(st.ghost_vox, np.int32), c(st.ghost_active, np.uint8)]
    m = max(n, 1)
    out = dict(owner=np.zeros((m, V), U32), dist=np.zeros((m, V), F), hc=np.zeros((m, L, 12), F), hcount=np.zeros((m, L), U32), ghost_active=np.zeros((m, L), np.uint8),
               ghost_done=np.zeros((m, L), np.uint8), tcnt=np.zeros((m, L), U32), n_changed=np.zeros(m, U32))
    rounds = np.zeros(m, U32); books = np.zeros((m, len(BOOKS)), U32); stats = np.zeros(4, U32); deep = np.zeros(2, U32)
    outs = list(out.values()) + [rounds, books, stats, deep]
    VP = ctypes.c_void_p
    w = np.array([st.seed_res, st.w_normal, st.w_color, st.w_spatial], F)
    f = emul.lib.f3ds_emul_sweeps_from
    f.restype = ctypes.c_int
    rc = f(ctypes.c_uint32(V), ctypes.c_uint32(st.S0), ctypes.c_uint32(n), (VP * 12)(*[a.ctypes.data for a in ins]), VP(w.ctypes.data), ctypes.c_int(inc_shift),
           ctypes.c_int(r_rounds), (VP * 12)(*[a.ctypes.data for a in outs]))
    assert rc == 0, "f3ds_emul_sweeps_from returned %d" % rc
    r = EmulRun()
    r.snap = {k: v[:n] for k, v in out.items()}
    r.stats = stats; r.r_deep, r.r_deep_cold = int(deep[0]), int(deep[1]); r.rounds = rounds[:n]
    r.books = {k: books[:n, i] for i, k in enumerate(BOOKS)}
    return r


ARRAYS = ("owner", "dist", "hc", "hcount", "ghost_active", "ghost_done", "tcnt", "n_changed")


def first_difference(got, want, ref_hcount):
    """None, or (sweep, array, index, got word, want word) of the first word in which two runs' snapshots differ -- sweep by sweep, arrays in the order of ARRAYS; the
    hc rows of helpers the reference has erased (hcount 0) are not compared: such a row is stale on the device by design; NaN matches NaN (conftest.same_bits)"""
    n = len(want["owner"])
    for t in range(n):
        for k in ARRAYS:
            a = np.ascontiguousarray(got[k][t]); b = np.ascontiguousarray(want[k][t]).astype(a.dtype)
            if k == "hc":
                keep = ref_hcount[t] > 0
                a = a[keep]; b = b[keep]
            if a.dtype.kind == "f":
                nan = np.isnan(a) & np.isnan(b)
                a = a.view(U32); b = b.view(U32)
                bad = np.flatnonzero(((a != b) & ~nan).reshape(-1))
            else:
                bad = np.flatnonzero((a != b).reshape(-1))
            if len(bad):
                i = int(bad[0])
                return t, k, i, int(a.reshape(-1)[i]), int(b.reshape(-1)[i])
    return None


def describe(case, diff, who="device", ref="literal reference"):
    t, k, i, a, b = diff
    return "case '%s': first difference in sweep %d, array %s, index %d: %s %08x, %s %08x" % (case, t, k, i, who, a, ref, b)


# ------------------------------------------------------------------------------------------------ the cases
class Case:
    def __init__(self, name, family, build, n=6, inc_shift=6, r_rounds=R_ROUNDS, cond=None, lead=False):
        self.name, self.family, self.build, self.n, self.inc_shift, self.r_rounds, self.cond, self.lead = name, family, build, n, inc_shift, r_rounds, cond, lead
        self._st = None

    @property
    def state(self):
        if self._st is None:
            self._st = self.build()
        return self._st

    def __repr__(self):
        return self.name


def _random_state(lat, S0, seed):
    """a random multi-leaf partition (a third of the voxels nobody's), random finite distances, random centroids that are not the leaves' means (what refine's reseed
    produces)"""
    rng = np.random.default_rng(seed)
    V = lat.V
    vf = features(lat, rng)
    owner = rng.integers(1, S0 + 1, V)
    if S0 == V:
        owner = rng.permutation(V) + 1
    owner[rng.random(V) < 0.3] = 0
    dist = rng.uniform(0.0, 2.0, V).astype(F)
    hc = np.zeros((S0 + 1, 12), F)
    pick = rng.integers(0, V, S0 + 1)
    hc[:, 0:3] = lat.xyz[pick] + rng.uniform(-2, 2, (S0 + 1, 3)).astype(F) * F(PITCH)
    hc[:, 3:6] = rng.uniform(0, 255, (S0 + 1, 3))
    n = rng.normal(size=(S0 + 1, 3)); hc[:, 6:9] = n / np.linalg.norm(n, axis=1, keepdims=True)
    return State(lat, vf, S0, owner, dist, hc)


def _uniform(lat, S0, owned, dist=0.0, hc_of=None, ghosts=None, **kw):
    """uniform colour and normals; owned: {label: voxels}; hc_of: {label: voxel whose feature row is the helper's start centroid} (default: its first voxel)"""
    vf = features(lat)
    owner = np.zeros(lat.V, np.int64)
    d = np.zeros(lat.V, F)
    hc = np.zeros((S0 + 1, 12), F)
    for h, vs in owned.items():
        vs = np.atleast_1d(vs)
        owner[vs] = h
        if len(vs):
            hc[h] = vf[vs[0]]
    d[:] = dist if np.isscalar(dist) else np.asarray(dist, F)
    for h, v in (hc_of or {}).items():
        hc[h] = vf[v]
    for h, v in (ghosts or {}).items():
        if h not in (hc_of or {}):
            hc[h] = vf[v]
    return State(lat, vf, S0, owner, d, hc, ghosts=ghosts, **kw)


def _far(st, h, rgb=(250.0, 5.0, 5.0)):
    """helper h's start centroid gets a colour far from every voxel's: it wins nothing in sweep 0"""
    st.hc[h, 3:6] = rgb
    return st


def _chain(n, descending):
    """a corridor of n voxels, one helper each, labels ascending (descending) along the ordinals, every start distance above what the neighbour offers: the helper of
    the lowest label keeps its voxel and takes the next, whose helper therefore takes nothing, whose neighbour keeps its voxel ... R(u_i) = not R(u_i-1)"""
    lat = corridor(n)
    lab = np.arange(n, 0, -1) if descending else np.arange(1, n + 1)
    return _uniform(lat, n, {int(lab[i]): [i] for i in range(n)}, dist=1.0)


def _books_16_17():
    """V = 1024 <= 48 S0: the row path.  Helper 1 holds pairs of voxels in tiles 0..14 and gains voxel 960 in tile 15: 16 raw entries, a row.  Helper 2 holds pairs in tiles
    0..15 and gains voxel 992: 17 raw entries, a wave.  Every other voxel belongs to wall helpers at distance 0."""
    lat = corridor(1024)
    owned = {}
    wall = 3 + np.arange(1024) // 40
    for h in np.unique(wall):
        owned[int(h)] = np.flatnonzero(wall == h)
    st = _uniform(lat, int(wall.max()), owned)
    one = np.concatenate([[64 * i + 62, 64 * i + 63] for i in range(15)]); two = np.concatenate([[64 * i + 30, 64 * i + 31] for i in range(16)])
    st.owner[one] = 1; st.owner[two] = 2; st.owner[[960, 992]] = 0
    st.dist[[960, 992]] = FLT_MAX
    st.hc[1] = st.vf[960]; st.hc[2] = st.vf[992]
    st.books()
    return st


def _sixty_five_tiles():
    lat = corridor(65 * 64 + 10)
    st = _uniform(lat, 2, {1: np.arange(65) * 64, 2: [65 * 64 + 9]})
    return st


def _plane_gain():
    """a 20 x 20 plane owned by helper 1 beside 20 x 20 cells nobody owns: 400 voxels gained in sweep 0"""
    lat = Lattice(block_cells(20, 20, 2))
    return _uniform(lat, 1, {1: np.flatnonzero(lat.cells[:, 2] == 0)})


def _raw_overflow():
    """d_sweep_claim appends one list entry per helper and 64-voxel tile it gained in, so a list only overflows when a helper gains in more than HT_CAP tiles in one
    sweep: no frame under HT_CAP * 64 = 16 384 voxels can.  The smallest shape found: a 36 x 32 x 16 block (18 432 voxels), helper 1 on the corner cell of every other
    4 x 4 x 4 block (32 tiles), gaining around each of them in 288 tiles at once."""
    lat = Lattice(block_cells(36, 32, 16))
    c = lat.cells
    return _uniform(lat, 1, {1: np.flatnonzero((c[:, 0] % 8 == 4) & (c[:, 1] % 8 == 4) & (c[:, 2] % 8 == 4))})


def _grow_64_65():
    """helper 1 holds 63 voxels at one end of a corridor and gains one per sweep: 64, 65, 66 leaves; V = 200 <= 48 S0 keeps the row path open"""
    lat = corridor(200)
    owned = {1: np.arange(63)}
    for h in range(2, 6):
        owned[h] = [194 + h]
    return _uniform(lat, 5, owned)


def _two_ends(n):
    lat = corridor(n)
    rng = np.random.default_rng(n)
    st = _uniform(lat, 2, {1: [0], 2: [n - 1]})
    st.vf[:, 3:6] = rng.integers(100, 140, (n, 3))          # colours that move the centroids, and with them the border between the two
    st.hc[1] = st.vf[0]; st.hc[2] = st.vf[n - 1]
    return st


def _tie_at(ulps):
    """helper 1 (voxels 0..3) offers voxel 4 exactly its distance (ulps = 0: no theft) or one ulp less than it holds (ulps = 1: theft)"""
    lat = corridor(8)
    st = _uniform(lat, 2, {1: np.arange(4), 2: np.arange(4, 8)}, dist=0.0, seed_res=16 * PITCH)
    d = voxel_distance(st.hc[1], st.vf[4], st.seed_res, st.w_normal, st.w_color, st.w_spatial)[0]
    st.dist[4] = d if ulps == 0 else np.nextafter(d, F(np.inf), dtype=F)
    assert st.dist[4] > 0
    return _far(st, 2)          # (helper 2, whose turn comes later, must not take the voxel back)


def _owner_is(t, v, h):
    return lambda run: None if run.ref["owner"][t, v] == h else "voxel %d belongs to %d after sweep %d, not to %d" % (v, run.ref["owner"][t, v], t, h)


def _all(*conds):
    def f(run):
        for c in conds:
            r = c(run)
            if r:
                return r
    return f


def _book(key, test, what):
    return lambda run: None if test(run.emul.books[key]) else "books[%s] = %s: %s" % (key, run.emul.books[key].tolist(), what)


def _cases():
    out = []
    # ---- A: shapes
    for V in (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513):
        for shape, lat_of in (("corridor", corridor), ("block", near_cube)):
            for S0 in sorted({1, 2, V}):
                out.append(Case("A %s V=%d S0=%d" % (shape, V, S0), "A", (lambda V=V, S0=S0, lat_of=lat_of: _random_state(lat_of(V), S0, 1000 * V + S0)),
                                lead=(V == 257 and S0 == 2 and shape == "block")))
    for V in (96, 97):          # V on either side of 48 S0: d_centroid's row path and a wave per helper
        out.append(Case("A block V=%d S0=2" % V, "A", (lambda V=V: _random_state(near_cube(V), 2, 7 * V)),
                        cond=_book("row" if V == 96 else "wave", lambda b: b[0] == 2, "both helpers on the %s path in sweep 0" % ("row" if V == 96 else "wave"))))
    # ---- B: exact ties
    out.append(Case("B equal distance: no theft", "B", lambda: _tie_at(0), cond=_all(_owner_is(0, 4, 2), lambda run: None if run.ref["ties"] >= 1 else "no tie"), lead=True))
    out.append(Case("B one ulp above: theft", "B", lambda: _tie_at(1), cond=_owner_is(0, 4, 1)))
    out.append(Case("B identical centroids", "B", lambda: _uniform(corridor(3), 2, {1: [0], 2: [2]}, hc_of={1: 1, 2: 1}), cond=_owner_is(0, 1, 1)))

    def plane():
        lat = Lattice(block_cells(9, 5, 3))
        return _uniform(lat, 2, {1: [lat.at(1, 2, 1)], 2: [lat.at(7, 2, 1)]})
    out.append(Case("B uniform block, mirror helpers", "B", plane, n=8, cond=lambda run: None if run.ref["ties"] >= 9 else "%d ties" % run.ref["ties"]))
    # ---- C: ghost leaves
    ghost = lambda t, h, on: (lambda run: None if bool(run.ref["ghost_active"][t, h]) == on else "ghost of helper %d %s after sweep %d" % (h, "inactive" if on else "active", t))
    out.append(Case("C one ghost", "C", lambda: _uniform(corridor(10), 2, {2: [5]}, ghosts={1: 5}, dist=0.5), cond=_all(_owner_is(0, 5, 1), ghost(0, 1, False)), lead=True))
    out.append(Case("C chain of two ghosts", "C", lambda: _far(_uniform(corridor(10), 3, {3: [5]}, ghosts={1: 5, 2: 5}), 1), n=5,
                    cond=lambda run: None if run.emul.stats[FULL] >= 3 else "the ghosts did not keep the sweeps full"))
    out.append(Case("C ghost voxel stolen by a third helper", "C", lambda: _far(_uniform(corridor(10), 3, {1: [4], 3: [5]}, ghosts={2: 5}, dist=1.5, hc_of={1: 5}), 2),
                    cond=_all(_owner_is(0, 5, 1), ghost(0, 2, True))))
    out.append(Case("C ghost helper wins its voxel", "C", lambda: _uniform(Lattice(block_cells(4, 4, 4)), 2, {2: [21]}, ghosts={1: 21}, dist=1.0),
                    cond=_all(_owner_is(0, 21, 1), ghost(0, 1, False))))
    out.append(Case("C ghost on ordinal 127", "C", lambda: _uniform(corridor(300), 2, {2: [127]}, ghosts={1: 127}, dist=0.5), cond=_owner_is(0, 127, 1)))
    out.append(Case("C ghosts that stay", "C", lambda: _uniform(corridor(40), 4, {2: [10], 4: [30]}, ghosts={1: 10, 3: 30}, dist=0.0), n=6,
                    cond=_all(ghost(5, 1, True), ghost(5, 3, True), lambda run: None if run.emul.stats[FULL] == 6 else "a sweep with ghost leaves was not full")))
    # ---- D: books
    out.append(Case("D plane gains 400", "D", _plane_gain, n=3,
                    cond=_all(_book("max_gain", lambda b: b[0] == 400, "400 voxels gained in sweep 0"),
                              _book("raw_overflow", lambda b: not b.any(), "a gain is one list entry per 64-voxel tile: 400 voxels of a plane are far from HT_CAP tiles")), lead=True))
    out.append(Case("D raw list overflows", "D", _raw_overflow, n=2, cond=_all(_book("raw_overflow", lambda b: b[0] == 1, "the HT_CAP overflow in sweep 0"),
                                                                              _book("max_raw", lambda b: b[0] > HT_CAP, "more than HT_CAP raw entries"))))
    out.append(Case("D leaves in 65 tiles", "D", _sixty_five_tiles, n=3, cond=_book("window", lambda b: b[0] >= 1, "the window scan in sweep 0")))
    out.append(Case("D 16 and 17 list entries", "D", _books_16_17, n=3,
                    cond=_all(_book("max_raw", lambda b: b[0] == 17, "17 raw entries"), _book("row", lambda b: b[0] >= 1, "row path"), _book("wave", lambda b: b[0] >= 1, "wave path"),
                              lambda run: None if run.ref["tcnt"][0, 1] == 16 and run.ref["tcnt"][0, 2] == 16 else "tile counts")))
    out.append(Case("D from 64 to 65 leaves", "D", _grow_64_65, n=5,
                    cond=lambda run: None if {64, 65} <= set(run.ref["hcount"][:, 1].tolist()) and run.emul.books["row"].sum() and run.emul.books["wave"].sum() else "hcount %s" % run.ref["hcount"][:, 1]))
    out.append(Case("D last leaf lost", "D", lambda: _uniform(corridor(12), 2, {1: [4], 2: [5]}, dist=1.5, hc_of={1: 5}), n=5,
                    cond=lambda run: None if run.ref["hcount"][0, 2] == 0 and run.ref["hcount"][4, 2] == 0 else "helper 2 still has leaves"))
    # ---- E: R dependencies
    for n in (3, 4, 5, 6, 23, 24, 25, 26, 200):
        # The voxel of the lowest label has no thief and is settled by the pre-pass; the n - 1 others form one chain of unsettled voxels.  The walker's stack holds
        # F3DS_R_STACK of them, the voxel it started from included (a_eval_R_mask: sp + 1 >= F3DS_R_STACK puts it off): n - 1 <= 24 fits, 26 voxels do not.
        deep = n - 1 > R_STACK
        out.append(Case("E chain %d descending" % n, "E", (lambda n=n: _chain(n, True)), n=3, inc_shift=-1, lead=(n == 200),
                        cond=_all(lambda run, deep=deep: None if (run.emul.r_deep > 0) == deep else "r_deep = %d" % run.emul.r_deep,
                                  _book("tail", lambda b, deep=deep: (b[0] > 0) == deep, "the tail kernel has work exactly above the stack"))))
        out.append(Case("E chain %d ascending" % n, "E", (lambda n=n: _chain(n, False)), n=3, inc_shift=-1,
                        cond=lambda run, deep=deep: None if run.emul.r_deep == 0 and (run.emul.r_deep_cold > 0) == deep else "r_deep = %d, cold %d" % (run.emul.r_deep, run.emul.r_deep_cold)))
    wraps = lambda run: None if run.emul.stats.sum() == 130 and run.ref["n_changed"][127:].any() else "the run went quiet before the tag wrapped twice: %s" % run.ref["n_changed"][120:]
    out.append(Case("E 130 full sweeps", "E", lambda: _two_ends(300), n=130, inc_shift=-1, cond=_all(wraps, lambda run: None if run.emul.stats[FULL] == 130 else "stats")))
    out.append(Case("E 130 default sweeps", "E", lambda: _two_ends(300), n=130, cond=_all(wraps, lambda run: None if run.emul.stats[INCREMENTAL] > 60 else "stats %s" % run.emul.stats)))
    return out


CASES = _cases()
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)


class Run:
    """a case's literal reference and emulation, computed once and shared by the tests that need them"""
    _cache = {}

    @classmethod
    def of(cls, emul, case):
        if case.name not in cls._cache:
            r = cls()
            r.ref = expand(case.state, case.n)
            r.emul = emul_from(emul, case.state, case.n, case.inc_shift, case.r_rounds)
            cls._cache[case.name] = r
        return cls._cache[case.name]


# ------------------------------------------------------------------------------------------------ states outside the contract (refused by kp_sweeps without a GPU)
def violations():
    """[(what, state)]: one breach of the start-state contract each"""
    base = lambda: _uniform(corridor(200), 3, {1: np.arange(0, 70), 2: np.arange(70, 140), 3: [150]}, ghosts={1: 100}, dist=0.25)
    out = []

    def add(what, f):
        st = base(); f(st); out.append((what, st))

    add("owner above S0", lambda s: s.owner.__setitem__(5, 4))
    add("neighbour index V", lambda s: s.nbr.__setitem__((3, 14), s.V))
    add("neighbour index below -1", lambda s: s.nbr.__setitem__((3, 0), -2))
    add("slot 13 is not the voxel", lambda s: s.nbr.__setitem__((3, 13), 4))
    add("neighbour table not symmetric", lambda s: s.nbr.__setitem__((3, 14), 9))
    add("hcount without the ghost leaf", lambda s: s.hcount.__setitem__(1, 70))
    add("hlo above a leaf", lambda s: s.hlo.__setitem__(2, 71))
    add("hhi below a leaf", lambda s: s.hhi.__setitem__(2, 100))
    add("hhi = V", lambda s: s.hhi.__setitem__(2, s.V))
    add("window of an empty helper", lambda s: (s.owner.__setitem__(150, 0), s.dist.__setitem__(150, FLT_MAX), s.hcount.__setitem__(3, 0)))
    add("tile list misses a tile", lambda s: s.tcnt.__setitem__(2, 1))
    add("tile list entry = T", lambda s: (s.tl.__setitem__((3, 1), 4), s.tcnt.__setitem__(3, 2)))
    add("tcnt above HT_CAP + 1", lambda s: s.tcnt.__setitem__(3, HT_CAP + 2))
    add("ghost on a voxel of a lower label", lambda s: (s.ghost_vox.__setitem__(3, 10), s.ghost_active.__setitem__(3, 1), s.hcount.__setitem__(3, 2), s.hlo.__setitem__(3, 10)))
    add("ghost on its own voxel", lambda s: s.ghost_vox.__setitem__(1, 5))
    add("ghost on a voxel nobody owns", lambda s: (s.ghost_vox.__setitem__(1, 160), s.hhi.__setitem__(1, 160)))
    add("ghost voxel = V", lambda s: s.ghost_vox.__setitem__(1, s.V))
    add("ghost voxel without ghost_active", lambda s: (s.ghost_active.__setitem__(1, 0), s.hcount.__setitem__(1, 70)))
    add("ghost_active = 255", lambda s: s.ghost_active.__setitem__(1, 255))
    add("a ghost leaf of label 0", lambda s: (s.ghost_vox.__setitem__(0, 100), s.ghost_active.__setitem__(0, 1)))
    add("distance of an unowned voxel", lambda s: s.dist.__setitem__(180, 1.0))
    add("negative distance", lambda s: s.dist.__setitem__(5, -0.5))
    add("distance NaN", lambda s: s.dist.__setitem__(5, np.nan))
    add("distance infinite", lambda s: s.dist.__setitem__(5, np.inf))
    add("centroid NaN", lambda s: s.hc.__setitem__((2, 4), np.nan))
    add("centroid infinite", lambda s: s.hc.__setitem__((0, 0), np.inf))
    add("feature NaN", lambda s: s.vf.__setitem__((7, 2), np.nan))
    add("seed_res 0", lambda s: setattr(s, "seed_res", 0.0))
    add("negative weight", lambda s: setattr(s, "w_color", -1.0))
    return out


BAD_CONTROLS = [dict(n=141), dict(r_rounds=0), dict(r_rounds=R_ROUNDS + 1), dict(tiles=2), dict(gx_cap=2), dict(inc_shift=-2), dict(inc_shift=33)]
