"""f3ds_region_shapes_host (include/f3ds.h, "region shapes") through ctypes against the reference of tests/region_shapes_common.py, bit for bit, the
properties of a converged decomposition, and every argument error.  No GPU: the library loads without one.

Shapes: the region table's (97 x 61 u16 tight, 67 x 45 f32 with padded depth rows, 3 x 2, 1 x 1).  Scenes: the table's 1 ... 9 (tests/test_region_table_cpu.py)
and
  "8+2"    scene 8's clamped depths under one region      every f_z^2 is 2^62: M_zz leaves 64 bits (asserted), sums kept in 64 bits cannot pass
  "tilted" one region on an oblique plane                  (a) the ordinary use: a normal, a small eigenvalue[0]
  "flat"   one region at one constant f32 depth            (a) N_zz == 0 exactly: cov[5] is the bits of +0.0
  "thin"   a column, one pixel, two pixels, the rest       (b) rank 1 and rank 0: the zero-off-diagonal skips and the stable tie order
  "mirror" two halves of a roof, mirrored in x             (c) the sign rules of normal and axis"""
import ctypes

import numpy as np
import pytest

import region_shapes_common as S
import region_table_common as R
from region_table_common import NO

ALL_SCENES = R.SCENES + S.EXTRA


def c_shapes(P, fmt, depth, labels, n_regions, layout="tight", fill=0xA5):
    """f3ds_region_shapes_host on raw buffers: (rc, rows, result); rows prefilled with `fill` bytes"""
    lib = P.load_library()
    f, dbuf, _ = R.buffers(fmt, depth, None, layout)
    lab = np.ascontiguousarray(labels, np.uint32).reshape(-1)
    rows = np.frombuffer(bytes([fill]) * (84 * int(n_regions)), P.REGION_SHAPE_DTYPE).copy()
    res = P.RegionShapesResult(7, 7, 7, 7)
    rc = lib.f3ds_region_shapes_host(ctypes.byref(f), dbuf.ctypes.data, lab.ctypes.data, int(n_regions), rows.ctypes.data if len(rows) else None, ctypes.byref(res))
    return rc, rows, res


def check(P, sc, key, layout):
    """the host function against the reference on one scene; returns (rows, the reference's result and moments)"""
    rc, rows, res = c_shapes(P, sc["fmt"], sc["depth"], sc["labels"], sc["n_regions"], layout)
    wrc, wrows, wres, moments = S.reference(P, key, sc)
    assert rc == wrc == 0
    S.assert_rows_equal(P, rows, wrows, "%r %s" % (key, layout))
    assert res.as_dict() == wres, (res.as_dict(), wres)
    return rows, wres, moments


@pytest.mark.parametrize("which", ALL_SCENES)
@pytest.mark.parametrize("width,height,depth_kind,layout", R.SHAPES)
def test_scene_equals_reference(P, width, height, depth_kind, layout, which):
    sc = S.any_scene(P, which, width, height, depth_kind)
    rows, res, moments = check(P, sc, (which, width, height, depth_kind), layout)
    n = rows["n_pixels"].astype(np.int64)
    assert int(n.sum()) == res["n_labelled"] and int((n > 0).sum()) == res["n_nonempty"]
    assert (S.words_of(rows[n == 0]) == np.array([0] + [R.QNAN] * 20, np.uint32)).all()
    big = width * height > 6
    if which == "8+2" and big:
        nn, _, M, _ = moments[0]
        assert res["n_clamped"] > 0 and M[5] > 2 ** 64 and nn * 2 ** 62 >= M[5] > (nn // 2) * 2 ** 62      # most z clamp at 32768 m: f_z^2 = 2^62 each
        if (width, height) == (97, 61):
            assert M[5] > 2 ** 73
    if which == "flat":
        w = S.words_of(rows)[0]
        assert w[9] == 0 and moments[0][3][5] == 0.0                               # cov zz: the bits of +0.0
        if big:
            assert w[10] == 0 and tuple(rows[0]["normal"]) == (0.0, 0.0, -1.0) and rows[0]["plane_d"] == rows[0]["centroid"][2]      # eigenvalue[0] is +0.0 too
    if which == "thin" and big:
        assert rows[1]["n_pixels"] == 1 and (S.words_of(rows)[1, 4:13] == 0).all() and tuple(rows[1]["normal"]) in ((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0))
        assert rows[1]["curvature"] == 0 and rows[0]["eigenvalue"][1] <= 2.0 ** -20 * rows[0]["eigenvalue"][2]      # one point: rank 0; the column: rank 1
        assert rows[2]["n_pixels"] == 2 and rows[2]["eigenvalue"][1] == 0 and rows[2]["eigenvalue"][2] > 0
    if which == "mirror" and big:
        a, b = rows[0], rows[1]
        flip = np.array([-1, 1, 1], np.float32)
        assert a["n_pixels"] == b["n_pixels"] and np.array_equal(a["centroid"] * flip, b["centroid"]) and np.array_equal(a["cov"][[0, 3, 4, 5]], b["cov"][[0, 3, 4, 5]])
        assert np.array_equal(a["cov"][[1, 2]], -b["cov"][[1, 2]]) and a["normal"][0] * b["normal"][0] < 0 and a["normal"][2] < 0 and b["normal"][2] < 0


@pytest.mark.parametrize("which", [1, "tilted", "flat", "mirror"])
@pytest.mark.parametrize("width,height,depth_kind,layout", R.SHAPES[:2])
def test_properties_of_the_rows(P, width, height, depth_kind, layout, which):
    """A convergence check that the reference alone passes as well (asserted): eigenvalues ascending and non-negative, unit vectors, the normal towards the
    camera, the eigen-residual, the eigenvalues against numpy.linalg.eigvalsh; and n_pixels and centroid are the region table's words."""
    sc = S.any_scene(P, which, width, height, depth_kind)
    rows, res, moments = check(P, sc, (which, width, height, depth_kind), layout)
    S.properties(S.reference(P, (which, width, height, depth_kind), sc)[1], moments)
    S.properties(rows, moments)
    trows, tres = P.region_table_host(sc["depth"], sc["labels"], sc["n_regions"], sc["fmt"])
    assert np.array_equal(S.words_of(rows)[:, 0], R.words_of(trows)[:, 0]) and np.array_equal(S.words_of(rows)[:, 1:4], R.words_of(trows)[:, 12:15])
    assert tres.as_dict() == res


@pytest.mark.parametrize("width,height,depth_kind,layout", R.SHAPES[:2])
def test_a_permutation_of_the_labels_permutes_the_rows(P, width, height, depth_kind, layout):
    for which in (1, 4, 6):
        sc = R.scene(P, which, width, height, depth_kind)
        K = sc["n_regions"]
        perm = np.random.default_rng(5).permutation(K).astype(np.uint32)
        lab = sc["labels"]
        moved = np.where(lab == NO, np.uint32(NO), perm[np.minimum(lab, K - 1)]).astype(np.uint32)
        rc0, rows0, res0 = c_shapes(P, sc["fmt"], sc["depth"], lab, K, layout)
        rc1, rows1, res1 = c_shapes(P, sc["fmt"], sc["depth"], moved, K, layout)
        assert rc0 == rc1 == 0 and res0.as_dict() == res1.as_dict()
        S.assert_rows_equal(P, rows1[perm], rows0)


@pytest.mark.parametrize("seed", R.RANDOM_SEEDS[:8])
def test_random_scene(P, seed):
    sc, _, layout = R.random_case(P, seed)
    check(P, sc, ("random", seed), layout)


def test_package_function(P):
    sc = R.scene(P, 1, 67, 45, "u16")
    rows, res = P.region_shapes_host(sc["depth"], sc["labels"], sc["n_regions"], sc["fmt"])
    wrows, wres = S.reference(P, (1, 67, 45, "u16"), sc)[1:3]
    S.assert_rows_equal(P, rows, wrows)
    assert res.as_dict() == wres and rows.dtype == P.REGION_SHAPE_DTYPE and ctypes.sizeof(P.RegionShape) == 84 == P.REGION_SHAPE_DTYPE.itemsize
    wide = np.zeros((45, 80), np.uint16); wide[:, :67] = sc["depth"]      # a view of a wider image: the row stride becomes the pitch
    S.assert_rows_equal(P, P.region_shapes_host(wide[:, :67], sc["labels"], sc["n_regions"], sc["fmt"])[0], wrows)
    with pytest.raises(P.F3dsError):
        P.region_shapes_host(sc["depth"], np.where(sc["labels"] == 0, 99, sc["labels"]), sc["n_regions"], sc["fmt"])


# ---- errors: the region table's list ------------------------------------------------------------------------------------------------------------------------

def test_argument_errors(P):
    lib = P.load_library()
    sc = R.scene(P, 1, 3, 2, "u16")
    fmt, K = R.with_color(P, sc["fmt"], "rgb8"), sc["n_regions"]
    d, l = sc["depth"], sc["labels"]
    rows = np.zeros(K, P.REGION_SHAPE_DTYPE)
    good = [ctypes.byref(fmt), d.ctypes.data, l.ctypes.data, K, rows.ctypes.data, None]      # NULL result
    assert lib.f3ds_region_shapes_host(*good) == 0
    for k in (0, 1, 2, 4):
        a = list(good); a[k] = None
        assert lib.f3ds_region_shapes_host(*a) == P.ERR_ARG, k
    for fields in (dict(width=0), dict(height=0), dict(depth_type=7), dict(fx=0.0), dict(fy=float("nan")), dict(depth_scale=0.0), dict(depth_scale=-1.0),
                   dict(cx=float("inf")), dict(cy=float("nan")), dict(depth_pitch=3), dict(depth_pitch=7)):
        f = fmt.copy()
        for k, v in fields.items():
            setattr(f, k, v)
        a = list(good); a[0] = ctypes.byref(f)
        assert lib.f3ds_region_shapes_host(*a) == P.ERR_ARG, fields
    for fields in (dict(color_format=99), dict(color_pitch=8)):                    # the colour fields are not looked at
        f = fmt.copy()
        for k, v in fields.items():
            setattr(f, k, v)
        a = list(good); a[0] = ctypes.byref(f)
        assert lib.f3ds_region_shapes_host(*a) == 0, fields
    a = list(good); a[3] = 0x01000000
    big = np.zeros(1, P.REGION_SHAPE_DTYPE)
    a[4] = big.ctypes.data                                                          # (refused before a row is touched)
    assert lib.f3ds_region_shapes_host(*a) == P.ERR_UNSUPPORTED
    a[4] = None
    assert lib.f3ds_region_shapes_host(*a) == P.ERR_ARG                             # NULL rows come first
    # n_regions == 0: rows may be NULL; any label but F3DS_NO_LABEL is then out of range
    none = np.full((2, 3), NO, np.uint32)
    res = P.RegionShapesResult(7, 7, 7, 7)
    assert lib.f3ds_region_shapes_host(ctypes.byref(fmt), d.ctypes.data, none.ctypes.data, 0, None, ctypes.byref(res)) == 0
    assert res.as_dict() == dict(n_regions=0, n_nonempty=0, n_labelled=0, n_clamped=0)
    assert lib.f3ds_region_shapes_host(ctypes.byref(fmt), d.ctypes.data, l.ctypes.data, 0, None, None) == P.ERR_ARG
    # a frame without a labelled pixel: every row empty
    rc, rows, res = c_shapes(P, fmt, np.zeros((2, 3), np.uint16), l, K)
    assert rc == 0 and res.as_dict() == dict(n_regions=K, n_nonempty=0, n_labelled=0, n_clamped=0)
    assert (S.words_of(rows) == np.array([0] + [R.QNAN] * 20, np.uint32)).all()


@pytest.mark.parametrize("width,height,depth_kind,layout", R.SHAPES)
def test_a_bad_label_leaves_the_rows_untouched(P, width, height, depth_kind, layout):
    sc = R.scene(P, 1, width, height, depth_kind)
    K = sc["n_regions"]
    for where, value, invalid_depth in ((-1, K, False), (0, K + 5, False), (-1, 0xFFFFFFFE, True)):
        lab = sc["labels"].copy(); lab.reshape(-1)[where] = value
        depth = sc["depth"].copy()
        if invalid_depth:
            depth.reshape(-1)[where] = 0                                            # out of range is out of range, whatever the depth
        rc, rows, res = c_shapes(P, sc["fmt"], depth, lab, K, layout)
        assert rc == P.ERR_ARG == S.ref_shapes(P, sc["fmt"], depth, lab, K)[0]
        assert (rows.view(np.uint8) == 0xA5).all() and res.as_dict() == dict(n_regions=7, n_nonempty=7, n_labelled=7, n_clamped=7)
