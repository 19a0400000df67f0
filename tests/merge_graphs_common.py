"""Synthetic supervoxel graphs for the merge loop (d_merge_il_t<NW, RES> and d_merge, csrc/f3ds_kernels.inc), and a structural replay of the oracle's merge log.

Plain numpy, no GPU.  make_graph() builds (sv, pairs) in the form Context.cluster_supervoxels / the oracle's cluster_supervoxels entry take; replay() walks
the oracle's EDGES + MERGES on region adjacency sets -- it is NOT a second implementation of the weights: it says how many adjacencies a merge touched, how many
of them were duplicates, how big the absorbed region was and how the next merge relates to it, and it checks the log against SV_REGION.  CASES lists every graph
with the kernel path it is for and the condition (check_condition) the oracle's run has to meet for the case to exercise that path: tests/test_merge_graphs_cpu.py
asserts each condition, tests/test_merge_graphs_gpu.py runs each case through the HIP merge loop.

replay()'s nt is deg(a) + deg(b) - 1; the kernels' touched list leaves the merged adjacency itself out and holds nt - 1 entries (touched()), so the star that fills the
list of MC_TL_CAP entries exactly has 1 025 spokes and the first that falls back to d_merge 1 026.

How the weights are steered.  Every supervoxel is a lattice of >= 4 voxels (coplanar, not collinear: a region of one or two voxels gets a degenerate PCA normal
after its first merge and merging stops) on the plane z = 1 with the normal (0, 0, 1) and a centroid on that plane, so delta_g = 0 for every edge and a weight is
lambda * CIEDE2000(mean colours) / range: the colours decide the order.  Two edges whose (lower label, higher label) colour pairs are equal have bit-equal weights.
Under ADAPTIVE_LAMBDA identical normals give lambda = 0 and every initial weight 0 (a mass tie); identical normals AND colours give lambda = NaN and no merge."""
import collections
import functools

import numpy as np

# ---- the constants of the merge kernels the cases are sized by (checked against the library's own by test_merge_graphs_cpu.py)
MC_TL_CAP = 1024        # adjacencies the two regions of one merge may touch in d_merge_il_t; also equal minimum keys its tie path takes
MC_SP_TL = 256          # adjacencies a speculative second merge may touch
MC_SP_LEAVES = 8        # supervoxels the region a speculative second merge absorbs may consist of
MC_GROUP = 16           # edge slots per order-key group
MC_LDS_LIMIT = 160 * 1024 - 2560
CHUNK_ROWS = {4: 128, 8: 256}      # rows per staging buffer, by waves per frame
SP_ROWS8_MAX = 1024     # rows a speculative second merge may fold in the 8-wave layout while LDS has room (128 with 4 waves)
SP_REST_TRIES, SP_REST_DIV, SP_REST_EPOCHS = 64, 4, 256      # the speculation rests for 256 epochs when fewer than 1 in 4 of the last 64 attempts were committed
EV_MULT, EV_EXTRA = 64, 4096       # weight-history events a frame starts with: E * 64 + 4096
LANES = 64

KERNEL_CONSTANTS = {       # name of P.constant() -> the value the cases assume
    "MC_TL_CAP": MC_TL_CAP, "MC_SP_TL": MC_SP_TL, "MC_SP_LEAVES": MC_SP_LEAVES, "MC_GROUP": MC_GROUP, "MC_SP_ROWS8": SP_ROWS8_MAX, "MC_SP_REST_DIV": SP_REST_DIV,
    "MC_CH_ROWS4": CHUNK_ROWS[4], "MC_CH_ROWS8": CHUNK_ROWS[8], "MC_SP_ROWS_MIN": 128, "MC_SP_REST_TRIES": SP_REST_TRIES, "MC_SP_REST_EPOCHS": SP_REST_EPOCHS,
    "MC_LDS_STATIC": 2560, "MC_LDS_LIMIT": MC_LDS_LIMIT, "EV_MULT": EV_MULT, "EV_EXTRA": EV_EXTRA,
    "OVF_EVENTS": 1, "OVF_LEAF_POOL": 2, "OVF_ILIST_POOL": 4,      # the reasons for a rerun of the merge stage
}


# ------------------------------------------------------------------------------------------------ building blocks
STEP = np.float32(0.004)        # lattice pitch of a supervoxel's voxels


def _assemble(n_vox, rgb, cen_xy, edges, normal=None, tilt=None):
    """Supervoxels 1..S (label = row + 1): n_vox[i] voxels on a lattice beside (cen_xy[i], 1), all of colour rgb[i]; edges: (i, j) rows.  tilt[i] lifts the
    voxels (not the given centroid) out of the plane by tilt * x offset.  pairs lists every edge in both directions, ordered like the multimap (by first label)."""
    n_vox = np.asarray(n_vox, np.int64); S = len(n_vox)
    rgb = np.asarray(rgb, np.uint32).reshape(S, 3)
    off = np.zeros(S + 1, np.uint32); off[1:] = np.cumsum(n_vox)
    V = int(off[-1])
    owner = np.repeat(np.arange(S), n_vox)
    j = np.arange(V) - off[:-1][owner].astype(np.int64)
    side = np.ceil(np.sqrt(np.maximum(n_vox, 4))).astype(np.int64)[owner]
    ox = (j % side).astype(np.float32) * STEP; oy = (j // side).astype(np.float32) * STEP
    cen = np.concatenate([np.asarray(cen_xy, np.float32).reshape(S, 2), np.ones((S, 1), np.float32)], axis=1)
    xyz = cen[owner].copy()
    xyz[:, 0] += ox; xyz[:, 1] += oy
    if tilt is not None:
        xyz[:, 2] += np.asarray(tilt, np.float32)[owner] * ox
    packed = (rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]
    nrm = np.tile(np.array([0, 0, 1], np.float32), (S, 1)) if normal is None else np.asarray(normal, np.float32).reshape(S, 3)
    sv = dict(label=np.arange(1, S + 1, dtype=np.uint32), voxel_offset=off, voxel_xyz=xyz.astype(np.float32), voxel_rgba=packed[owner].astype(np.uint32),
              centroid_xyz=cen, normal=nrm)
    e = np.asarray(edges, np.int64).reshape(-1, 2) + 1
    both = np.vstack([e, e[:, ::-1]])
    both = both[np.lexsort((both[:, 1], both[:, 0]))]
    return sv, both.astype(np.uint32)


def kept_edges(pairs):
    """The adjacencies clear_adjacency keeps (first <= second), in the order they enter the weight map: EDGES of the oracle, slot order of the kernels."""
    return pairs[pairs[:, 0] < pairs[:, 1]]


def _far_colours(rng, n):
    """n colours, consecutive ones far apart (no accidental small weight between neighbours of a chain)."""
    out = np.zeros((n, 3), np.int64)
    prev = np.array([128, 128, 128])
    for i in range(n):
        while True:
            c = rng.integers(0, 256, 3)
            if np.abs(c - prev).sum() >= 90:
                break
        out[i] = c; prev = c
    return out


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _chain_xy(n, x0=0.0, y=0.0):
    return np.stack([x0 + np.arange(n) * 0.1, np.full(n, y)], axis=1)


def _chain_edges(n, first=0):
    return [(first + i, first + i + 1) for i in range(n - 1)]


# ------------------------------------------------------------------------------------------------ the graph kinds
def g_star(rng, spokes, close=40, hub_vox=400, tilt=0.0, tail=0):
    """Hub (label 1) with `spokes` leaves.  `close` spokes differ from the hub's colour by little (distinct small steps: they merge), the others by much.  tilt: the hub's
    voxels lie on a tilted plane while every given normal is (0, 0, 1): all initial delta_g are 0, after the first merge the hub's PCA normal is no longer exactly
    (0, 0, 1) and its adjacencies weigh more than 0 (without the tilt a star of equal keys keeps merging at weight 0 to the end: 7 s of oracle time for 1 099 spokes).
    tail: a separate chain of that many supervoxels on the plane (keeps merging at delta_g = 0)."""
    S = 1 + spokes + tail
    rgb = np.zeros((S, 3), np.int64)
    rgb[0] = (128, 128, 128)
    far = _far_colours(rng, spokes)
    far[np.abs(far - 128).sum(axis=1) < 60] = (250, 20, 30)
    rgb[1:1 + spokes] = far
    which = rng.permutation(spokes)[:close]
    for k, s in enumerate(which):       # distinct small colour steps around the hub's grey
        rgb[1 + s] = (128 + (k % 7) - 3, 128 + ((k // 7) % 7) - 3, 128 + (k // 49) - 1)
    if tail:
        rgb[1 + spokes:] = rng.integers(0, 256, (tail, 3))
    ang = np.arange(spokes) * (2 * np.pi / spokes)
    xy = np.zeros((S, 2)); xy[1:1 + spokes, 0] = 3.0 * np.cos(ang); xy[1:1 + spokes, 1] = 3.0 * np.sin(ang)
    if tail:
        xy[1 + spokes:] = _chain_xy(tail, 10.0, 10.0)
    n_vox = np.full(S, 4); n_vox[0] = hub_vox
    edges = [(0, 1 + s) for s in range(spokes)] + _chain_edges(tail, 1 + spokes)
    tl = np.zeros(S); tl[0] = tilt
    return _assemble(n_vox, rgb, xy, edges, tilt=tl if tilt else None)


def g_grid(rng, w, h, colours="random", n_vox=4, ties=(), tie_pair=((100, 100, 100), (102, 101, 100)), low_pair=None, big=None, normals="flat", pad=0):
    """4-connected w x h grid, row-major labels.  colours: 'random' | 'equal'.  ties: horizontal edges (row, col) -> (row, col + 1) that get the colour pair tie_pair;
    low_pair: ((row, col), colour pair) one more horizontal edge with a smaller weight still; big: ((row, col), voxels) one supervoxel of another size.
    normals: 'flat' (0, 0, 1) everywhere | 'varied' (random tilts: distinct delta_g, for ADAPTIVE_LAMBDA)."""
    S = w * h
    idx = lambda r, c: r * w + c
    rgb = rng.integers(0, 256, (S, 3)) if colours == "random" else np.tile(np.array([90, 120, 60]), (S, 1))
    for (r, c) in ties:
        rgb[idx(r, c)] = tie_pair[0]; rgb[idx(r, c + 1)] = tie_pair[1]
    if low_pair is not None:
        (r, c), pr = low_pair
        rgb[idx(r, c)] = pr[0]; rgb[idx(r, c + 1)] = pr[1]
    nv = np.full(S, n_vox)
    if big is not None:
        nv[idx(*big[0])] = big[1]
    xy = np.stack([np.tile(np.arange(w), h) * 0.1, np.repeat(np.arange(h), w) * 0.1], axis=1)
    edges = [(idx(r, c), idx(r, c + 1)) for r in range(h) for c in range(w - 1)] + [(idx(r, c), idx(r + 1, c)) for r in range(h - 1) for c in range(w)]
    if pad:       # a separate chain of `pad` edges behind the grid: any edge count
        rgb = np.vstack([rgb, _far_colours(rng, pad + 1)]); nv = np.concatenate([nv, np.full(pad + 1, n_vox)])
        xy = np.vstack([xy, _chain_xy(pad + 1, 0.0, -5.0)]); edges += _chain_edges(pad + 1, S)
        S += pad + 1
    nrm = None
    if normals == "varied":
        nrm = _unit(np.concatenate([rng.normal(0, 0.25, (S, 2)), np.ones((S, 1))], axis=1))
    return _assemble(nv, rgb, xy, edges, normal=nrm)


TIE_PAIR = ((100, 100, 100), (102, 101, 100))
LOW_PAIR = ((60, 60, 60), (61, 60, 60))


def tie_slots(k, placement):
    """Edge slots (= chain positions) of k equal keys, three slots apart at the least (a chain edge between two tie edges would join the same two colours and tie as well).
    'group': five to a 16-slot group from group 2 on: k <= 5 lie in ONE group; 'lane': five to a group, in groups 64 apart (2, 66, 130, 194: the same lane of wave 0 holds
    their minima); 'lanes': every key in another group, three groups apart (different lanes)."""
    if placement == "group":
        return [32 + 1 + 3 * (i % 5) + 16 * (i // 5) for i in range(k)]
    if placement == "lane":
        per = 5 if k > 3 else 1
        return [32 + 1 + 3 * (i % per) + 1024 * (i // per) for i in range(k)]
    if placement == "lanes":
        return [32 + 3 + 48 * i for i in range(k)]
    raise ValueError(placement)


def g_tie_chain(rng, k, placement, runner_up=False, normals="flat", n=None):
    """A chain in which exactly k edges (tie_slots) carry the colour pair TIE_PAIR -- the smallest weight of the graph, or with runner_up the second smallest behind one
    edge of LOW_PAIR at slot 8 -- and every other edge joins far colours.  normals 'paired': unit normals tilted in the y-z plane (the chain runs along x, so N.C = 0 and
    delta_g = |N1 x N2| / 3), the same pair on every tie edge, another on the low edge and random ones elsewhere: distinct delta_g for ADAPTIVE_LAMBDA / EQUALIZATION, ties kept."""
    slots = tie_slots(k, placement)
    n = n or (max(slots) + 40)
    rgb = _far_colours(rng, n)
    tilt = rng.uniform(-0.5, 0.5, n)
    for s in slots:
        rgb[s] = TIE_PAIR[0]; rgb[s + 1] = TIE_PAIR[1]; tilt[s] = 0.05; tilt[s + 1] = 0.09
    if runner_up:
        rgb[8] = LOW_PAIR[0]; rgb[9] = LOW_PAIR[1]; tilt[8] = -0.02; tilt[9] = -0.03
    nrm = None
    if normals == "paired":
        nrm = _unit(np.stack([np.zeros(n), np.sin(tilt), np.cos(tilt)], axis=1))
    return _assemble(np.full(n, 4), rgb, _chain_xy(n), _chain_edges(n), normal=nrm)


def g_chain(rng, n, n_vox=4, normals="flat"):
    nrm = None
    if normals == "varied":
        t = rng.uniform(-0.5, 0.5, n)
        nrm = _unit(np.stack([np.zeros(n), np.sin(t), np.cos(t)], axis=1))
    return _assemble(np.full(n, n_vox), rng.integers(0, 256, (n, 3)), _chain_xy(n), _chain_edges(n), normal=nrm)


def g_nan_chain(rng, n=64, at=30):
    sv, pairs = g_chain(rng, n)
    sv["normal"][at] = np.nan
    return sv, pairs


def g_clique(rng, n, normals="flat"):
    ang = np.arange(n) * (2 * np.pi / n)
    xy = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    nrm = None
    if normals == "varied":
        nrm = _unit(np.concatenate([rng.normal(0, 0.25, (n, 2)), np.ones((n, 1))], axis=1))
    return _assemble(np.full(n, 4), rng.integers(0, 256, (n, 3)), xy, [(i, j) for i in range(n) for j in range(i + 1, n)], normal=nrm)


BIG_SIZES = [1, 127, 128, 129, 255, 256, 257, 511, 513, 1023, 1025, 1100]


def g_big_single(rng, sizes=BIG_SIZES):
    """Chain a0 B0 a1 B1 ...: B_i holds sizes[i] voxels and almost a_i's colour (the edge merges, B_i is absorbed as one leaf); B_i -> a_{i+1} joins far colours."""
    base = _far_colours(rng, len(sizes))
    rgb, nv = [], []
    for i, s in enumerate(sizes):
        rgb += [base[i], np.clip(base[i] + (1 + i % 3, i % 2, 0), 0, 255)]; nv += [4, s]
    n = len(nv)
    return _assemble(nv, rgb, _chain_xy(n), _chain_edges(n))


def g_big_leaves(rng, leaves=(7, 8, 9, 7, 8, 9)):
    """Segments a, b1 .. bk of one chain: the b's differ by a grey step or less and merge among themselves first (region b1 of k leaves), a differs from them by a few steps more and
    absorbs that region afterwards.  Between segments the colours are far apart."""
    base = _far_colours(rng, len(leaves))
    base = np.clip(base, 20, 235)
    rgb = []
    for i, k in enumerate(leaves):
        rgb.append(base[i] + (7, 5, 3))
        for j in range(k):
            rgb.append(base[i] + ((j * 3) % 2, (j * 5) % 2, (j // 2) % 2))
    n = len(rgb)
    return _assemble(np.full(n, 6), rgb, _chain_xy(n), _chain_edges(n))


def g_chains(rng, count, length, normals="flat"):
    """`count` disjoint chains with random colours; labels interleaved (supervoxel j of chain c is row j * count + c), so neighbouring slots belong to different chains."""
    S = count * length
    edges = [((j) * count + c, (j + 1) * count + c) for c in range(count) for j in range(length - 1)]
    xy = np.stack([(np.arange(S) // count) * 0.1, (np.arange(S) % count) * 1.0], axis=1)
    nrm = None
    if normals == "varied":
        t = rng.uniform(-0.5, 0.5, S)
        nrm = _unit(np.stack([np.zeros(S), np.sin(t), np.cos(t)], axis=1))
    return _assemble(np.full(S, 4), rng.integers(0, 256, (S, 3)), xy, edges, normal=nrm)


def g_monotone_chain(rng, n=22, normals="flat"):
    """Greys 128 - 3, 128 + 6, 128 - 9, ... behind a first supervoxel of 2000 voxels at 128 (the growing region's mean stays there): supervoxel k is 3 k from the region and
    3 (2 k + 1) from its successor, so the cheapest edge is always the one next to the region that has just grown."""
    g = 128 + 3 * np.arange(n) * (-1) ** np.arange(n)
    rgb = np.stack([g, g, g], axis=1)
    nrm = None
    if normals == "varied":
        t = np.linspace(0.0, 0.4, n) ** 2
        nrm = _unit(np.stack([np.zeros(n), np.sin(t), np.cos(t)], axis=1))
    nv = np.full(n, 4); nv[0] = 2000
    return _assemble(nv, rgb, _chain_xy(n), _chain_edges(n), normal=nrm)


def g_ladder(rng, rungs, chains=0, length=0, normals="flat"):
    """Rungs (2i, 2i + 1) of two almost equal colours, cheaper from rung to rung by a growing step; rails between neighbouring rungs join far colours.  The two cheapest edges are
    always neighbouring rungs, joined by the rails (the speculation's s_cross).  Behind the ladder `chains` disjoint chains of random colours."""
    base = [np.array((40, 60, 200)), np.array((200, 150, 30))]      # even and odd rungs: far apart, so the rails are dear
    rgb = []
    for i in range(rungs):
        rgb += [base[i % 2], base[i % 2] + (0, (2 if i % 2 else 3) * (1 + i), 0)]      # (a green step weighs 1.5 times as much at the second base)
    nl = 2 * rungs
    edges = [(2 * i, 2 * i + 1) for i in range(rungs)] + [(2 * i + s, 2 * i + 2 + s) for i in range(rungs - 1) for s in (0, 1)]
    xy = [((i // 2) * 0.1, (i % 2) * 0.1) for i in range(nl)]
    S = nl + chains * length
    for c in range(chains):
        for j in range(length):
            rgb.append(rng.integers(0, 256, 3)); xy.append((j * 0.1, 5.0 + c))
        edges += _chain_edges(length, nl + c * length)
    nrm = None
    if normals == "varied":
        t = rng.uniform(-0.3, 0.3, S)
        nrm = _unit(np.stack([np.sin(t), np.zeros(S), np.cos(t)], axis=1))
    return _assemble(np.full(S, 4), rgb, xy, edges, normal=nrm)


def g_rest(rng, pairs=70, big=1100, chains=8, length=60):
    """`pairs` disjoint edges (a_i, B_i) of almost equal colours, B_i of `big` voxels -- more than a speculative second merge may fold in any layout, so every attempt
    with such a runner-up stands down --, then `chains` disjoint chains of small supervoxels with random colours (dearer edges: they merge afterwards)."""
    rgb, xy, nv, edges = [], [], [], []
    base = _far_colours(rng, pairs)
    for i in range(pairs):
        rgb += [base[i], np.clip(base[i] + (1 if base[i][0] < 255 else -1, 0, 0), 0, 255)]; xy += [(0.5 * i, 0.0), (0.5 * i, 0.2)]; nv += [4, big]
        edges.append((2 * i, 2 * i + 1))
    first = 2 * pairs
    far = _far_colours(rng, chains * length)
    for c in range(chains):
        for j in range(length):
            k = c * length + j
            rgb.append(far[k] if j % 2 == 0 else np.clip(far[k - 1] + rng.integers(4, 30, 3), 0, 255)); xy.append((0.1 * j, 5.0 + c)); nv.append(4)
        edges += _chain_edges(length, first + c * length)
    return _assemble(nv, rgb, xy, edges)


def g_hubs(rng,degrees=(300, 300, 230), close=30, normals="flat"):
    """Several stars side by side; `close` spokes of each differ little from their hub (distinct steps, interleaved between the hubs by the random draw)."""
    rgb, xy, nv, edges = [], [], [], []
    hubs = [(128, 128, 128), (60, 160, 90), (200, 90, 150)]
    for h, d in enumerate(degrees):
        hub = len(rgb)
        rgb.append(hubs[h]); xy.append((10.0 * h, 0.0)); nv.append(300)
        far = _far_colours(rng, d)
        far[np.abs(far - hubs[h]).sum(axis=1) < 60] = (250, 250, 10)
        which = set(rng.permutation(d)[:close].tolist())
        for s in range(d):
            k = rng.integers(0, 10 ** 6)
            col = np.array(hubs[h]) + ((k % 9) - 4, ((k // 9) % 9) - 4, ((k // 81) % 9) - 4) if s in which else far[s]
            rgb.append(col); xy.append((10.0 * h + 3 * np.cos(s * 2 * np.pi / d), 3 * np.sin(s * 2 * np.pi / d))); nv.append(4)
            edges.append((hub, hub + 1 + s))
    S = len(rgb)
    nrm = None
    if normals == "varied":
        nrm = _unit(np.concatenate([rng.normal(0, 0.2, (S, 2)), np.ones((S, 1))], axis=1))
    return _assemble(nv, rgb, xy, edges, normal=nrm)


KINDS = dict(star=g_star, grid=g_grid, tie_chain=g_tie_chain, chain=g_chain, nan_chain=g_nan_chain, clique=g_clique, big_single=g_big_single, big_leaves=g_big_leaves,
             chains=g_chains, monotone_chain=g_monotone_chain, ladder=g_ladder, hubs=g_hubs, rest=g_rest)


def make_graph(kind, seed=0, **kw):
    """(sv, pairs) of one synthetic graph, deterministic from (kind, seed, kw)."""
    return KINDS[kind](np.random.default_rng(seed), **kw)


# ------------------------------------------------------------------------------------------------ structural replay
Replay = collections.namedtuple("Replay", "nt dups rows_b leaves_b relation n_regions reweighted")


def replay(edges, merges, sv, sv_region=None, n_regions=None):
    """Replay EDGES (E x 2 labels) and MERGES (M x 3: a, b, weight bits) on region adjacency sets.  Per merge: nt = deg(a) + deg(b) - 1 (the adjacencies the merge touches
    besides its own), dups = common neighbours of a and b (one of each pair of adjacencies is dropped), rows_b / leaves_b = voxels / supervoxels of the absorbed region,
    relation of the NEXT merge to this one: 'shares' (a region in common), 'adjacent' (disjoint, but an adjacency joins the two merges), 'independent', None after the last.
    Raises AssertionError when a merge does not join two alive, adjacent regions, or when the final partition / region count differ from sv_region / n_regions."""
    labels = [int(l) for l in sv["label"]]
    rows = dict(zip(labels, np.diff(sv["voxel_offset"]).astype(np.int64).tolist()))
    leaves = {l: [l] for l in labels}
    adj = {l: set() for l in labels}
    for a, b in np.asarray(edges).reshape(-1, 2).tolist():
        assert a in adj and b in adj and a != b, "edge (%d, %d) of unknown or equal labels" % (a, b)
        adj[a].add(b); adj[b].add(a)
    m = np.asarray(merges).reshape(-1, 3)[:, :2].tolist()
    nt, dups, rows_b, leaves_b, relation, rew = [], [], [], [], [], []
    for k, (a, b) in enumerate(m):
        assert a in adj and b in adj, "merge %d: (%d, %d) joins a region that is gone" % (k, a, b)
        assert a < b and b in adj[a], "merge %d: (%d, %d) are not adjacent, or not (lower, higher)" % (k, a, b)
        if k + 1 < len(m):
            a2, b2 = m[k + 1]
            if a2 in (a, b) or b2 in (a, b):
                relation.append("shares")
            elif (adj[a] | adj[b]) & {a2, b2}:
                relation.append("adjacent")
            else:
                relation.append("independent")
        else:
            relation.append(None)
        common = (adj[a] & adj[b])
        nt.append(len(adj[a]) + len(adj[b]) - 2); dups.append(len(common))
        rew.append(nt[-1] - dups[-1])
        rows_b.append(rows[b]); leaves_b.append(len(leaves[b]))
        for x in adj[b]:
            adj[x].discard(b)
            if x != a:
                adj[x].add(a); adj[a].add(x)
        adj[a].discard(b)
        del adj[b]
        rows[a] += rows.pop(b); leaves[a] += leaves.pop(b)
    if n_regions is not None:
        assert len(adj) == int(n_regions), "replay ends with %d regions, the log says %d" % (len(adj), n_regions)
    if sv_region is not None:
        root = {}
        for r, ls in leaves.items():
            for l in ls:
                root[l] = r
        want = [root[l] for l in sorted(labels)]
        assert want == [int(x) for x in sv_region], "the partition of the replay differs from SV_REGION"
    return Replay(np.array(nt, np.int64) + 1, np.array(dups, np.int64), np.array(rows_b, np.int64), np.array(leaves_b, np.int64), relation, len(adj), np.array(rew, np.int64))


def touched(rp):
    """Entries of the kernels' touched list per merge: every adjacency of a or b but the merged one = nt - 1 (d_merge_il_t gives up above MC_TL_CAP of them)."""
    return rp.nt - 1


# ------------------------------------------------------------------------------------------------ the cases
MANUAL, ADAPTIVE, EQUALIZATION = 0, 1, 2
MODE_NAME = {MANUAL: "manual", ADAPTIVE: "adaptive", EQUALIZATION: "equalization"}
FIT_EDGES = 12096       # the largest E for which d_merge_il_t<8 waves, keys in LDS> fits (P.merge_layout_info; checked by the CPU test); sp_rows is 128 there
FIT_GRID = 78           # a 78 x 78 grid has 12 012 edges: a chain pads it to the edge count wanted

Case = collections.namedtuple("Case", "name family kind seed kw merging threshold cond layout variants envs cont")
# layout: what Context.merge_layout() has to say after the case -- 'lds' the layout that was asked for, (8, 2) by default; 'fallback' (0, 0) whatever was asked for (the
#         stage ran again with d_merge); 'global_keys' (8, 0) by default (E is too large for LDS keys);  variants: also run in all nine MERGE_VARIANTS;
# envs: further switch settings the case runs under; cont: recluster / labels_at_thresholds continue on its state
CASES = []


def case(name, family, kind, kw, merging, threshold, cond, layout="lds", variants=True, envs=(), cont=False, seed=0):
    CASES.append(Case(name, family, kind, seed, dict(kw), merging, float(threshold), cond, layout, variants, tuple(envs), cont))


def in_modes(name, family, kind, kw, thresholds, conds, kw_other=None, kw_adaptive=None, **rest):
    """The case under MANUAL_LAMBDA (flat normals: the colours decide), ADAPTIVE_LAMBDA and EQUALIZATION.  kw_other: what the graph takes instead under the other two modes
    (normals that differ: with flat ones lambda would be 0), kw_adaptive: under ADAPTIVE_LAMBDA alone."""
    for mode in (MANUAL, ADAPTIVE, EQUALIZATION):
        k = dict(kw)
        if mode != MANUAL and kw_other:
            k.update(kw_other)
        if mode == ADAPTIVE and kw_adaptive:
            k.update(kw_adaptive)
        case("%s-%s" % (name, MODE_NAME[mode]), family, kind, k, mode, thresholds[mode], conds[mode], **rest)


# 1. hub over the touched-list cap
case("star1099", 1, "star", dict(spokes=1099), MANUAL, 0.012, ("hub", 1098, 30, 60), layout="fallback")
case("star1024", 1, "star", dict(spokes=1024), MANUAL, 0.004, ("first_touched", 1023))
case("star1025", 1, "star", dict(spokes=1025), MANUAL, 0.004, ("first_touched", MC_TL_CAP))              # the list is exactly full: stays in LDS
case("star1026", 1, "star", dict(spokes=1026), MANUAL, 0.004, ("first_touched", MC_TL_CAP + 1), layout="fallback")
# 2. mass ties
case("star1099-all-equal", 2, "star", dict(spokes=1099, tilt=0.3, tail=120), ADAPTIVE, 1e-6, ("mass_tie", 120), layout="fallback", cont=True)
# (every epoch of an all-equal grid is a tie among all that is left, walked by one thread: 0.1 s of kernel time for 12 x 12, 1.1 s for 22 x 22 -- the larger one runs once)
in_modes("grid12-all-equal", 2, "grid", dict(w=12, h=12, colours="equal"), {MANUAL: 0.2, ADAPTIVE: 0.2, EQUALIZATION: 1.5},
         {m: ("mass_tie", 143) for m in (MANUAL, ADAPTIVE, EQUALIZATION)}, kw_adaptive=dict(colours="random"), cont=True)      # (one colour AND one normal would give lambda = NaN)
case("grid22-all-equal", 2, "grid", dict(w=22, h=22, colours="equal"), MANUAL, 0.2, ("mass_tie", 483), variants=False)          # 924 equal keys: the most the tie path takes itself
case("grid30-all-equal", 2, "grid", dict(w=30, h=30, colours="equal"), MANUAL, 0.2, ("mass_tie", 899), layout="fallback")      # 1 740 equal keys: the tie path's own fallback
# 3. sparse ties: 2, 3, 17 equal keys in one group / one lane's groups / different lanes, as the minimum and as the runner-up
for _k in (2, 3, 17):
    for _pl in ("group", "lane", "lanes"):
        for _ru in (False, True):
            in_modes("tie%d-%s-%s" % (_k, _pl, "second" if _ru else "min"), 3, "tie_chain", dict(k=_k, placement=_pl, runner_up=_ru), {MANUAL: 0.02, ADAPTIVE: 0.02, EQUALIZATION: 0.3},
                     {MANUAL: ("sparse_tie", _k, _pl, 1 if _ru else 0), ADAPTIVE: ("sparse_tie", _k, _pl, 1 if _ru else 0), EQUALIZATION: ("equal_slots", _k, _pl)},
                     kw_other=dict(normals="paired"))
case("grid12-tie3", 3, "grid", dict(w=12, h=12, ties=((1, 1), (5, 7), (9, 3))), MANUAL, 0.02, ("grid_tie", 3, 0))
case("grid12-tie3-second", 3, "grid", dict(w=12, h=12, ties=((1, 1), (5, 7), (9, 3)), low_pair=((7, 1), LOW_PAIR)), MANUAL, 0.02, ("grid_tie", 3, 1))
# 4. more weight-history events than the arrays start with
case("star400-to-the-end", 4, "star", dict(spokes=400, hub_vox=4), MANUAL, 5.0, ("events",), cont=True)
# 5. duplicate adjacencies
in_modes("clique40", 5, "clique", dict(n=40), {MANUAL: 5.0, ADAPTIVE: 5.0, EQUALIZATION: 5.0}, {m: ("dups", 38) for m in (0, 1, 2)}, kw_other=dict(normals="varied"))
in_modes("clique12", 5, "clique", dict(n=12), {MANUAL: 5.0, ADAPTIVE: 5.0, EQUALIZATION: 5.0}, {m: ("dups", 10) for m in (0, 1, 2)}, kw_other=dict(normals="varied"))
# 6. big absorbed regions
case("big-single-leaves", 6, "big_single", {}, MANUAL, 0.02, ("rows", tuple(BIG_SIZES)), cont=True)
case("big-many-leaves", 6, "big_leaves", {}, MANUAL, 0.03, ("leaves", (7, 8, 9)), cont=True)
# 7. independent and dependent pairs of merges
in_modes("chains8x40", 7, "chains", dict(count=8, length=40), {MANUAL: 0.1, ADAPTIVE: 0.1, EQUALIZATION: 0.4}, {m: ("independent_half",) for m in (0, 1, 2)}, kw_other=dict(normals="varied"))
in_modes("monotone-chain", 7, "monotone_chain", {}, {MANUAL: 5.0, ADAPTIVE: 5.0, EQUALIZATION: 5.0}, {MANUAL: ("all_share",), ADAPTIVE: ("merges", 10), EQUALIZATION: ("merges", 10)},
         kw_other=dict(normals="varied"))
in_modes("ladder20", 7, "ladder", dict(rungs=20), {MANUAL: 0.07, ADAPTIVE: 0.07, EQUALIZATION: 0.5}, {MANUAL: ("cross", 7), ADAPTIVE: ("merges", 10), EQUALIZATION: ("merges", 10)},
         kw_other=dict(normals="varied"))
in_modes("hubs", 7, "hubs", {}, {MANUAL: 0.01, ADAPTIVE: 0.1, EQUALIZATION: 0.1}, {MANUAL: ("hubs",), ADAPTIVE: ("merges", 10), EQUALIZATION: ("merges", 10)}, kw_other=dict(normals="varied"))
case("rest-and-resume", 7, "rest", dict(chains=8, length=120), MANUAL, 0.06, ("rest", 70))
# 8. size edges
for _e in (1, 15, 16, 17, 63, 64, 65, 255, 256, 257):
    case("chain-E%d" % _e, 8, "chain", dict(n=_e + 1), MANUAL, 0.1 if _e > 1 else 5.0, ("edges", _e, 1), variants=False, envs=(dict(F3DS_MERGE_NW="4", F3DS_MERGE_KEYS="lds"),))
for _t in (512, 256):       # NGcap = groups rounded up to the workgroup's width T: 16 T - 1, 16 T, 16 T + 1 edges
    for _e in (16 * _t - 1, 16 * _t, 16 * _t + 1):
        case("chain-E%d" % _e, 8, "chain", dict(n=_e + 1), MANUAL, 0.03, ("edges", _e, 50), variants=False, envs=(dict(F3DS_MERGE_NW="4", F3DS_MERGE_KEYS="lds"), dict(F3DS_MERGE_NW="4", F3DS_MERGE_KEYS="global")))
_pad = FIT_EDGES - 2 * FIT_GRID * (FIT_GRID - 1)
case("grid-E%d-fits" % FIT_EDGES, 8, "grid", dict(w=FIT_GRID, h=FIT_GRID, pad=_pad), MANUAL, 0.025, ("edges", FIT_EDGES, 100), variants=False)
case("grid-E%d-global-keys" % (FIT_EDGES + 64), 8, "grid", dict(w=FIT_GRID, h=FIT_GRID, pad=_pad + 64), MANUAL, 0.025, ("edges", FIT_EDGES + 64, 100), layout="global_keys", variants=False)
case("grid-E%d-big-runner-up" % FIT_EDGES, 8, "grid", dict(w=FIT_GRID, h=FIT_GRID, pad=_pad, low_pair=((3, 3), LOW_PAIR), ties=((40, 40),), big=((40, 41), 129)), MANUAL, 0.025,
     ("big_runner_up", 129), variants=False)
# 9. NaN keys beside finite ones
case("nan-chain-manual", 9, "nan_chain", {}, MANUAL, 5.0, ("nan", 61, 3))
case("nan-chain-adaptive", 9, "nan_chain", {}, ADAPTIVE, 5.0, ("nan_lambda",))
# 10. every family once more under sparse 32-bit keys with permuted rows (relabel of test_cluster_supervoxels.py)
RELABELLED = ["star1099", "grid12-all-equal-manual", "tie17-lane-second-manual", "star400-to-the-end", "clique40-manual", "big-many-leaves", "rest-and-resume", "chain-E257", "nan-chain-manual"]

CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)


@functools.lru_cache(maxsize=None)
def graph_of(name):
    c = CASE[name]
    return make_graph(c.kind, c.seed, **c.kw)


def params_of(P, c):
    return P.default_params(merging=c.merging, threshold=c.threshold)


Run = collections.namedtuple("Run", "case sv pairs rc region vlab res h edges weights merges sv_region rp seconds")
_runs = {}


def oracle_run(oracle, P, name):
    """The oracle's run of a case, made once per process and shared (read-only) by every test that needs it."""
    if name not in _runs:
        import time
        c = CASE[name]
        sv, pairs = graph_of(name)
        t0 = time.perf_counter()
        rc, region, vlab, res, h = oracle.cluster_supervoxels(sv, pairs, params_of(P, c))
        dt = time.perf_counter() - t0
        assert rc == 0, "the oracle refuses case %s: %d" % (name, rc)
        edges, weights, merges, sv_region = h.get("EDGES").reshape(-1, 2), h.get("EDGE_WEIGHTS"), h.get("MERGES").reshape(-1, 3), h.get("SV_REGION")
        rp = replay(edges, merges, sv, sv_region, res.n_regions)      # (validates the log)
        _runs[name] = Run(c, sv, pairs, rc, region, vlab, res, h, edges, weights, merges, sv_region, rp, dt)
    return _runs[name]


# ------------------------------------------------------------------------------------------------ the conditions
def _bits(w):
    return np.ascontiguousarray(w, np.float32).view(np.uint32)


def check_condition(r, P=None):
    """Assert that the oracle's run r (oracle_run) of a case meets the case's structural condition: that it exercises the path it is for."""
    cond, rp, c = r.case.cond, r.rp, r.case
    what, args = cond[0], cond[1:]
    M = len(r.merges)
    assert r.res.n_merges == M and r.res.n_edges == len(r.edges)
    if what == "hub":                  # the first merge touches more adjacencies than the list holds; a few dozen merges follow
        assert touched(rp)[0] == args[0] > MC_TL_CAP and args[1] <= M <= args[2], (touched(rp)[:1], M)
    elif what == "first_touched":      # ... exactly so many, and no later merge more
        assert touched(rp)[0] == args[0] == touched(rp).max() and M >= 5, (touched(rp)[:3], M)
    elif what == "mass_tie":           # one weight for every edge; at least so many merges
        assert len(np.unique(_bits(r.weights))) == 1 and not np.isnan(r.weights).any() and M >= args[0], (len(np.unique(_bits(r.weights))), M)
        if c.layout == "fallback" and c.name != "star1099-all-equal":
            assert len(r.edges) > MC_TL_CAP
        if c.layout == "lds":
            assert len(r.edges) <= MC_TL_CAP and len(np.unique(r.merges[:, 2])) == 1      # every epoch is a tie among all that is left
    elif what in ("sparse_tie", "equal_slots"):
        k, placement = args[0], args[1]
        slots = np.array(tie_slots(k, placement))
        groups = slots // MC_GROUP
        if placement == "group" and k <= 5:
            assert len(set(groups.tolist())) == 1
        if placement == "lane":
            assert len(set((groups % LANES).tolist())) == 1 and (k <= 3) == (len(set(groups.tolist())) == k)
        if placement == "lanes":
            assert len(set((groups % LANES).tolist())) == min(k, LANES)
        wb = _bits(r.weights)
        assert len(set(wb[slots].tolist())) == 1, "the tie edges differ"
        tie_bits = int(wb[slots[0]])
        if what == "sparse_tie":       # exactly k edges at the smallest (rank 0) or second smallest (rank 1) weight, and exactly one below them at rank 1
            u = np.unique(r.weights)
            assert np.float32(u[args[2]]).view(np.uint32) == tie_bits and np.array_equal(np.nonzero(wb == tie_bits)[0], np.sort(slots)), (u[:3], np.nonzero(wb == tie_bits)[0])
            assert args[2] == 0 or int((r.weights == u[0]).sum()) == 1
            assert np.array_equal(r.merges[args[2]:args[2] + k, 2], np.full(k, tie_bits, np.uint32)), "the equal keys are not merged one after the other"
        assert int((r.merges[:, 2] == tie_bits).sum()) >= k, "not every tie edge was merged at its initial weight"
    elif what == "grid_tie":
        k, rank = args
        u = np.unique(r.weights)
        assert int((r.weights == u[rank]).sum()) == k and (rank == 0 or int((r.weights == u[0]).sum()) == 1)
        assert np.array_equal(r.merges[rank:rank + k, 2], np.full(k, np.float32(u[rank]).view(np.uint32)))
    elif what == "events":             # initial entries + re-weightings exceed the event arrays the context starts with
        E = len(r.edges)
        assert E + int(rp.reweighted.sum()) > EV_MULT * E + EV_EXTRA and M == E, (E, int(rp.reweighted.sum()))
    elif what == "dups":
        assert rp.dups.max() >= args[0] >= 10 and r.res.n_regions == 1, rp.dups.max()
    elif what == "rows":               # every size is absorbed once, as a single supervoxel
        assert sorted(rp.rows_b.tolist()) == sorted(args[0]) and set(rp.leaves_b.tolist()) == {1}, (rp.rows_b, rp.leaves_b)
    elif what == "leaves":             # absorbed regions of 7, 8, 9 supervoxels: either side of MC_SP_LEAVES
        assert set(args[0]) <= set(rp.leaves_b.tolist()) and min(args[0]) < MC_SP_LEAVES + 1 <= max(args[0]), rp.leaves_b
    elif what == "independent_half":
        assert rp.relation.count("independent") * 2 >= M >= 40, (M, rp.relation.count("independent"))
    elif what == "all_share":
        assert M >= 20 and all(x == "shares" for x in rp.relation[:-1]), rp.relation
    elif what == "cross":              # the two cheapest edges are joined by a third, args[0] times in a row from the first merge on
        assert all(x == "adjacent" for x in rp.relation[:args[0]]), rp.relation
    elif what == "hubs":               # independent neighbours in the log: a second merge with more than MC_SP_TL adjacencies, and one with fewer whose sum with the first exceeds 512 lanes
        t = touched(rp)
        ind = [k for k in range(M - 1) if rp.relation[k] == "independent"]
        assert any(t[k + 1] > MC_SP_TL for k in ind) and any(t[k + 1] <= MC_SP_TL and t[k] + t[k + 1] > 512 for k in ind), t[:40]
    elif what == "rest":               # `args[0]` independent merges whose absorbed region is too big for any speculative second merge, then more than 256 epochs, then independent small ones
        n = args[0]
        assert n > SP_REST_TRIES and (rp.rows_b[:n] > SP_ROWS8_MAX).all() and all(x == "independent" for x in rp.relation[:n - 1])
        later = rp.relation[n + SP_REST_EPOCHS:]
        assert later.count("independent") >= 64 and (rp.rows_b[n:] <= 128).all(), (M, later.count("independent"))
    elif what == "edges":
        assert len(r.edges) == args[0] and M >= args[1], (len(r.edges), M)
    elif what == "big_runner_up":      # the second merge absorbs a supervoxel of sp_rows + 1 voxels and has nothing to do with the first
        assert len(r.edges) == FIT_EDGES and rp.relation[0] == "independent" and rp.rows_b[1] == args[0] and rp.leaves_b[1] == 1 and M >= 100, (rp.relation[0], rp.rows_b[:3])
        if P is not None:
            assert P.merge_layout_info(FIT_EDGES, 8, 2)[1] + 1 == args[0]
    elif what == "nan":
        assert (M, r.res.n_regions) == (args[0], args[1]) and int(np.isnan(r.weights).sum()) == 2 and not np.isnan(r.merges[:, 2].view(np.float32)).any()
    elif what == "nan_lambda":
        assert M == 0 and np.isnan(r.res.lambda_) and np.isnan(r.weights).all()
    elif what == "merges":
        assert M >= args[0], M
    else:
        raise AssertionError("unknown condition %r" % (what,))
