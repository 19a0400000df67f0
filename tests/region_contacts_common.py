"""Shared by tests/test_region_contacts_cpu.py and tests/test_region_contacts_gpu.py: the numpy reference of the region contacts (include/f3ds.h, "region
contacts"), written from the definition -- depths and the class of a pair in np.float32 arithmetic, the fixed point with np.float64 / np.rint / int64, counts
and minima with np.add.at / np.minimum.at, the row order from np.unique over (a, b) -- and the scenes both files run.  It does not call the library.  Rows are
compared bit for bit as eight u32 words.

Scenes (1 ... 6 are the region table's, as they are):
   1 blocks of regions, 10 % holes, 5 % unlabelled       the ordinary path
   2 one region over the whole image                      zero rows
   3 every pixel its own region, n_regions = n            about two rows per pixel: overflows any LDS table and the first record buffer
   4 label = p mod 7                                      every pair a contact onto at most 21 rows: contention
   5 n_regions = 1000 over at most twelve labels          wide keys, few rows
   6 labels over invalid depths                           take part in nothing
   7 depth steps of three kinds along every border        close, a in front and b in front on one border
   8 gaps exactly on depth_tol * zn, one ulp either side  the threshold (f32 depths, depth_tol = 2^-4: the product is exact)
   9 depth_tol = 0                                        only equal depths are close
  10 gaps (2k + 1) / 2^17                                 the fixed point lands on .5: ties to even"""
import numpy as np

import region_table_common as R
import track_common as T
from rgbd_common import frame_format

NO = 0xFFFFFFFF
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_CAPACITY = 0, -1, -7, -10
SHAPES = R.SHAPES + [(40, 1, "u16", "tight"), (1, 40, "f32", "padded")]      # a single row has no lower neighbour anywhere, a single column no right one
SCENES = list(range(1, 11))
u32, f32, f64, i64 = np.uint32, np.float32, np.float64, np.int64
buffers = R.buffers


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------
def depth_z(fmt, depth):
    """(z (float32, flat), valid (bool, flat)) by the rule of f3ds_deproject: z = (f32)d * depth_scale in one rounded f32 product"""
    d = np.asarray(depth).reshape(-1)
    s = f32(fmt.depth_scale)
    with np.errstate(all="ignore"):
        if d.dtype == np.uint16:
            return d.astype(f32) * s, d != 0
        d = d.astype(f32)
        return d * s, (d > 0) & np.isfinite(d)


def pairs_of(fmt, depth, labels, depth_tol):
    """every contact pair of the definition: dict of flat arrays p (first pixel), q, horizontal, a, b, close, a_front, g (float32)"""
    h, w = int(fmt.height), int(fmt.width)
    lab = np.asarray(labels, u32).reshape(-1)
    z, valid = depth_z(fmt, depth)
    labelled = valid & (lab != NO)
    pix = np.arange(h * w, dtype=i64).reshape(h, w)
    p = np.concatenate([pix[:, :-1].reshape(-1), pix[:-1, :].reshape(-1)])
    q = np.concatenate([pix[:, :-1].reshape(-1) + 1, pix[:-1, :].reshape(-1) + w])
    hz = np.concatenate([np.ones(h * (w - 1), bool), np.zeros((h - 1) * w, bool)])
    m = labelled[p] & labelled[q] & (lab[p] != lab[q])
    p, q, hz = p[m], q[m], hz[m]
    p_is_a = lab[p] < lab[q]
    a, b = np.where(p_is_a, lab[p], lab[q]), np.where(p_is_a, lab[q], lab[p])
    za, zb = np.where(p_is_a, z[p], z[q]).astype(f32), np.where(p_is_a, z[q], z[p]).astype(f32)
    with np.errstate(all="ignore"):
        g = np.abs(za - zb)                              # one rounded f32 subtraction
        zn = np.where(za < zb, za, zb)
        bound = f32(depth_tol) * zn                      # one rounded f32 product
        close = g <= bound
    assert g.dtype == f32 and bound.dtype == f32
    return dict(p=p, q=q, horizontal=hz, a=a.astype(i64), b=b.astype(i64), close=close, a_front=~close & (za < zb), g=g, bound=bound)


def ref_contacts(P, fmt, depth, labels, n_regions, depth_tol):
    """(rc, rows (REGION_CONTACT_DTYPE), result dict) of the definition; rows and result are None unless rc == 0"""
    K = int(n_regions)
    lab = np.asarray(labels, u32).reshape(-1)
    if ((lab != NO) & (lab >= K)).any():
        return ERR_ARG, None, None
    c = pairs_of(fmt, depth, labels, depth_tol)
    ab = np.stack([c["a"], c["b"]], axis=1)
    uniq, inv = np.unique(ab, axis=0, return_inverse=True) if len(ab) else (np.zeros((0, 2), i64), np.zeros(0, i64))
    inv = np.asarray(inv).reshape(-1)
    rows = np.zeros(len(uniq), P.REGION_CONTACT_DTYPE)
    rows["a"], rows["b"] = uniq[:, 0], uniq[:, 1]
    cnt = {}
    for name, flag in (("n_pairs", np.ones(len(inv), bool)), ("n_close", c["close"]), ("n_a_front", c["a_front"]), ("n_horizontal", c["horizontal"])):
        cnt[name] = np.zeros(len(uniq), i64)
        np.add.at(cnt[name], inv, flag.astype(i64))
        rows[name] = cnt[name]
    first = np.full(len(uniq), NO, i64)
    np.minimum.at(first, inv, c["p"])
    rows["first_pixel"] = first
    fix = np.rint(np.minimum(c["g"].astype(f64), 32768.0) * 65536.0).astype(i64)
    s = np.zeros(len(uniq), i64)
    np.add.at(s, inv, fix)
    rows["mean_gap"] = ((s.astype(f64) / cnt["n_pairs"].astype(f64)) * 2.0 ** -16).astype(f32)
    return OK, rows, dict(n_regions=K, n_contacts=len(uniq), n_pairs=int(cnt["n_pairs"].sum()), n_close=int(cnt["n_close"].sum()))


def words_of(rows):
    return np.ascontiguousarray(rows).view(u32).reshape(len(rows), 8)


def assert_rows_equal(got, want, what=""):
    assert len(got) == len(want), "%s %d rows, want %d" % (what, len(got), len(want))
    g, w = words_of(got), words_of(want)
    if not np.array_equal(g, w):
        i, k = [int(a[0]) for a in np.nonzero(g != w)]
        raise AssertionError("%s row %d word %d: %#x, want %#x\ngot  %r\nwant %r" % (what, i, k, g[i, k], w[i, k], got[i], want[i]))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------------
def scene(P, which, width, height, depth_kind):
    """scene `which` (1 ... 10, the table of this file's docstring) at this size: dict(fmt, depth, labels (h, w) u32, n_regions, depth_tol)"""
    if which <= 6:
        return dict(R.scene(P, which, width, height, depth_kind), depth_tol=0.05)
    w, h = width, height
    rng = np.random.default_rng(100 * which + w)
    fmt = frame_format(P, w, h, "f32", "rgb8", 1.0)      # f32 depths in metres: every depth below is exact
    nx, ny = min(2, w), min(2, h)
    lab = T.blocks(w, h, nx, ny)
    uu, vv = np.meshgrid(np.arange(w), np.arange(h))
    kind = (uu + vv) % 3
    low = lab == 0                                       # block 0 keeps the base depth; the others step away from it
    if which == 7:      # close (1 mm), the base in front (1 m behind it), the base behind (1 m in front of it): all three along every border of block 0
        depth = np.where(low, 2.0, 2.0 + np.choose(kind, [0.001, 1.0, -1.0])).astype(f32)
        tol = 0.05
    elif which == 8:    # base 2 m, depth_tol 2^-4: the bound is 0.125 exactly; the other side at 2.125 (on it: close), one ulp nearer (close), one ulp further (not)
        on = f32(2.125)
        depth = np.where(low, f32(2.0), np.choose(kind, [on, np.nextafter(on, f32(0)), np.nextafter(on, f32(4))])).astype(f32)
        tol = 0.0625
    elif which == 9:    # depth_tol 0: equal depths are close, one ulp is not
        depth = np.where(low | (kind == 0), f32(2.0), np.nextafter(f32(2.0), f32(4))).astype(f32)
        tol = 0.0
    else:               # gaps (2k + 1) / 2^17 against the base of 1 m: g * 65536 = k + 0.5, towards even in both directions
        k = rng.integers(0, 1 << 12, (h, w))
        depth = np.where(low, f32(1.0), f32(1.0) + (2 * k + 1).astype(f32) / f32(131072.0)).astype(f32)
        tol = 0.05
    return dict(fmt=fmt, depth=depth, labels=lab.astype(u32), n_regions=int(nx * ny), depth_tol=tol)


def random_case(P, seed):
    """seeded random scene: (scene dict, layout); depth kind, layout and depth_tol chosen by the seed"""
    rng = np.random.default_rng(7000 + seed)
    w, h = [(67, 45), (97, 61), (40, 30)][seed % 3]
    depth_kind = "u16" if seed % 2 == 0 else "f32"
    K = int(rng.integers(1, 41))
    depth, lab = T.random_scene(rng, w, h, K, depth_kind)
    tol = float(rng.choice([0.0, 0.01, 0.05, 0.2]))
    return dict(fmt=T.track_format(P, w, h, depth_kind), depth=depth, labels=lab, n_regions=K, depth_tol=tol), "padded" if (seed // 2) % 2 else "tight"


RANDOM_SEEDS = list(range(18))
