"""f3ds_cloud_regions_host (include/f3ds.h, "region rows of a point cloud") through ctypes.  No GPU: the library loads without one.

1. Against the family: the records of f3ds_deproject under a scene's labels give the words of f3ds_region_table_host (n_pixels, first_pixel, lo, hi, centroid,
   mean_rgb), of f3ds_region_shapes_host (cov ... curvature) and of f3ds_region_boxes_host (every word of every row), and the three results.  Shapes and
   scenes: the region table's and the region shapes' (97 x 61 u16, 67 x 45 f32, 3 x 2, 1 x 1; scenes 1 ... 9, "8+2", "tilted", "flat", "thin", "mirror").
2. Against the reference of tests/cloud_regions_common.py on the clouds an image cannot reach (cloud_regions_common.CLOUDS).
3. A fixed shuffle of records and labels together keeps every bit but first_point, which becomes the minimum of the permuted indices.
4. Every error in the stated order, outputs prefilled with 0xA5 and found untouched.
5. The host code in a stand-alone program under the sanitizers (tests/cloud_regions_host_main.cpp)."""
import ctypes

import numpy as np
import pytest

import cloud_regions_common as C
import region_boxes_common as B
import region_shapes_common as S
import region_table_common as R
from region_table_common import NO

ALL_SCENES = R.SCENES + S.EXTRA
SEVENS = dict(n_regions=7, n_nonempty=7, n_labelled=7, n_clamped=7, n_inliers=7)


# ---- 1. against the family -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ALL_SCENES)
@pytest.mark.parametrize("width,height,depth_kind,layout", R.SHAPES)
def test_scene_as_a_cloud_equals_table_shapes_and_boxes(P, width, height, depth_kind, layout, which):
    sc, pts = C.scene_cloud(P, which, width, height, depth_kind)
    K, lab = sc["n_regions"], sc["labels"].reshape(-1)
    rc, rows, boxes, res = C.c_cloud(P, pts, lab, K)
    assert rc == 0
    trows, tres = P.region_table_host(sc["depth"], sc["labels"], K, sc["fmt"], color=sc["color"])
    srows, sres = P.region_shapes_host(sc["depth"], sc["labels"], K, sc["fmt"])
    brows, bres = P.region_boxes_host(sc["depth"], sc["labels"], K, sc["fmt"], plane_tol=C.TOL)
    w, tw, sw = C.words_of(rows), R.words_of(trows), S.words_of(srows)
    assert np.array_equal(w[:, 0], tw[:, 0]) and np.array_equal(w[:, 1], tw[:, 1])          # n_pixels, first_pixel
    assert np.array_equal(w[:, 2:14], tw[:, 6:18])                                          # lo, hi, centroid, mean_rgb
    assert np.array_equal(w[:, 0], sw[:, 0]) and np.array_equal(w[:, 8:11], sw[:, 1:4])     # n_pixels and the shapes' centroid
    assert np.array_equal(w[:, 14:31], sw[:, 4:21])                                         # cov, eigenvalue, normal, axis, plane_d, curvature
    assert (w[:, 31] == 0).all()
    B.assert_rows_equal(P, boxes, brows, "%r" % (which,))
    assert res.as_dict() == bres.as_dict()
    assert {k: res.as_dict()[k] for k in R.RESULT_FIELDS} == tres.as_dict() == sres.as_dict()
    # without boxes: the same rows, no inliers, the boxes untouched
    rc, rows2, boxes2, res2 = C.c_cloud(P, pts, lab, K, want_boxes=False)
    assert rc == 0 and (boxes2.view(np.uint8) == 0xA5).all() and res2.as_dict() == dict(res.as_dict(), n_inliers=0)
    C.assert_rows_equal(rows2, rows)


# ---- 2. against a reference of its own --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.CLOUDS + ["n%d" % n for n in C.LAUNCH_SIZES])
def test_cloud_equals_reference(P, name):
    c = C.cloud(name)
    wrc, wrows, wboxes, wres = C.reference(P, name)
    rc, rows, boxes, res = C.c_cloud(P, c["pts"], c["labels"], c["K"], c["tol"], c["fold"])
    assert rc == wrc == 0
    C.assert_rows_equal(rows, wrows, name)
    B.assert_rows_equal(P, boxes, wboxes, name + " boxes")
    assert res.as_dict() == wres, (res.as_dict(), wres)
    n = rows["n_points"].astype(np.int64)
    assert int(n.sum()) == wres["n_labelled"] and int((n > 0).sum()) == wres["n_nonempty"]
    assert (C.words_of(rows[n == 0]) == C.EMPTY_ROW).all() and (B.words_of(boxes[n == 0]) == B.EMPTY_ROW).all()


def test_what_the_edge_clouds_are_for(P):
    """the properties the clouds of item 2 were built to have, read off the host function's rows"""
    rows = lambda name: C.c_cloud(P, *[C.cloud(name)[k] for k in ("pts", "labels", "K", "tol", "fold")])
    rc, r, _, res = rows("empty")
    assert rc == 0 and res.as_dict() == dict(n_regions=4, n_nonempty=0, n_labelled=0, n_clamped=0, n_inliers=0) and (C.words_of(r) == C.EMPTY_ROW).all()
    rc, r, b, res = rows("one_point")
    assert rc == 0 and r["n_points"].tolist() == [0, 1] and r["first_point"].tolist() == [NO, 0] and r["mean_rgb"][1].tolist() == [128.0, 64.0, 32.0]
    assert (r["cov"][1] == 0).all() and (b["half"][1] == 0).all() and np.array_equal(r["lo"][1], r["hi"][1])
    rc, r, _, res = rows("one_region")
    assert rc == 0 and r["n_points"][0] == 500 == res.n_labelled
    rc, r, _, res = rows("one_coordinate_not_finite")
    assert rc == 0 and res.n_labelled == 40 - 6
    rc, r, _, _ = rows("signed_zero")
    w = C.words_of(r)
    assert w[0, 2] == w[0, 3] == 0x80000000 and w[0, 5] == w[0, 6] == 0 and w[1, 4] == 0x80000000 and w[1, 7] == 0 and w[1, 2] == 0x80000000 and w[1, 5] == 0
    rc, r, _, res = rows("clamped")
    assert rc == 0 and res.n_clamped == 4 and r["hi"][0][0] == np.float32(3.0e38) and r["lo"][0][1] == np.float32(-3.0e38)
    (_, r0, _, res0), (_, r1, _, res1) = rows("negative_z"), rows("negative_z_folded")
    assert res0.n_labelled == res1.n_labelled == 299 and (r0["lo"][:, 2] < 0).all() and (r1["lo"][:, 2] > 0).all()
    rc, r, _, res = rows("no_label_over_finite")
    assert rc == 0 and res.n_labelled == 40 and res.n_nonempty == 2 and r["n_points"][2] == 0
    rc, r, _, res = rows("labels_over_not_finite")
    assert rc == 0 and res.n_labelled == 30 and r["n_points"].tolist() == [30, 0]
    assert C.cloud("K3000")["K"] == 3000 and len(np.unique(C.cloud("K3000")["labels"][:256])) > 128      # scattered: one workgroup's trip meets more labels than a table holds


# ---- 3. permutation ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["K23", "K200", "negative_z_folded", "labels_over_not_finite", "clamped"])
def test_a_shuffle_keeps_every_bit_but_first_point(P, name):
    c = C.cloud(name)
    n = len(c["labels"])
    perm = np.random.default_rng(99).permutation(n)
    rc0, rows0, boxes0, res0 = C.c_cloud(P, c["pts"], c["labels"], c["K"], c["tol"], c["fold"])
    rc1, rows1, boxes1, res1 = C.c_cloud(P, c["pts"][perm], c["labels"][perm], c["K"], c["tol"], c["fold"])
    assert rc0 == rc1 == 0 and res0.as_dict() == res1.as_dict()
    assert np.array_equal(np.delete(C.words_of(rows1), 1, axis=1), np.delete(C.words_of(rows0), 1, axis=1))
    B.assert_rows_equal(P, boxes1, boxes0)
    where = np.empty(n, np.int64); where[perm] = np.arange(n)      # point i of the first cloud is point where[i] of the second
    idx, lab, _, _ = C.labelled_points(c["pts"], c["labels"], c["fold"])
    want = np.full(c["K"], NO, np.uint32)
    np.minimum.at(want, lab, where[idx].astype(np.uint32))
    assert np.array_equal(rows1["first_point"], want)


# ---- the package's wrappers ---------------------------------------------------------------------------------------------------------------------------------
def test_package_function(P):
    c = C.cloud("K23")
    _, wrows, wboxes, wres = C.reference(P, "K23")
    rows, res = P.cloud_regions_host(c["pts"], c["labels"], c["K"])
    C.assert_rows_equal(rows, wrows)
    assert res.as_dict() == dict(wres, n_inliers=0) and rows.dtype == P.CLOUD_REGION_DTYPE and ctypes.sizeof(P.CloudRegion) == 128 == P.CLOUD_REGION_DTYPE.itemsize
    rows, boxes, res = P.cloud_regions_host(c["pts"], c["labels"], c["K"], params=P.default_cloud_params(), want_boxes=True)
    C.assert_rows_equal(rows, wrows)
    B.assert_rows_equal(P, boxes, wboxes)
    assert res.as_dict() == wres
    d = P.default_cloud_params()
    assert (d.plane_tol, d.fold_negative_z) == (np.float32(0.01), 0) and P.default_cloud_params(fold_negative_z=1).fold_negative_z == 1
    rows, res = P.cloud_regions_host(np.zeros((0, 4), np.float32), np.zeros(0, np.uint32), 3)
    assert (C.words_of(rows) == C.EMPTY_ROW).all() and res.n_labelled == 0
    with pytest.raises(P.F3dsError):
        P.cloud_regions_host(c["pts"], np.where(c["labels"] == 0, 99, c["labels"]), c["K"])
    with pytest.raises(P.F3dsError):
        P.cloud_regions_host(c["pts"], c["labels"], c["K"], params=P.CloudParams(-1.0, 0))
    assert P.DBG_CLOUD_PATH == 25 and callable(P.Context.cloud_regions) and callable(P.cloud_regions_batch)


# ---- 4. errors, in the stated order -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_in_order(P):
    lib = P.load_library()
    c = C.cloud("n65")
    pts, lab, K = c["pts"], c["labels"], c["K"]
    rows = np.frombuffer(b"\xA5" * (128 * K), P.CLOUD_REGION_DTYPE).copy()
    boxes = np.frombuffer(b"\xA5" * (96 * K), P.REGION_BOX_DTYPE).copy()
    res = P.CloudRegionsResult(7, 7, 7, 7, 7)
    prm = P.CloudParams(0.01, 0)
    bad_lab = lab.copy(); bad_lab[3] = K
    call = lambda a: lib.f3ds_cloud_regions_host(*a)
    good = [pts.ctypes.data, len(lab), lab.ctypes.data, K, ctypes.byref(prm), rows.ctypes.data, boxes.ctypes.data, ctypes.byref(res)]

    def untouched():
        return (rows.view(np.uint8) == 0xA5).all() and (boxes.view(np.uint8) == 0xA5).all() and res.as_dict() == SEVENS

    def with_(**kw):
        a = list(good)
        for k, v in kw.items():
            a[dict(pts=0, n=1, lab=2, K=3, prm=4, rows=5, boxes=6, res=7)[k]] = v
        return a
    nan_tol, neg_tol = P.CloudParams(float("nan"), 0), P.CloudParams(-0.5, 0)
    # ARG: NULL labels, NULL points with n > 0, NULL rows with regions, a bad tolerance -- each also in front of what comes later in the order
    for a in (with_(lab=None), with_(pts=None), with_(rows=None), with_(prm=ctypes.byref(nan_tol)), with_(prm=ctypes.byref(neg_tol)), with_(prm=ctypes.byref(P.CloudParams(float("-inf"), 0))),
              with_(lab=None, K=0x01000000), with_(rows=None, K=0x01000000), with_(prm=ctypes.byref(neg_tol), K=0x01000000), with_(prm=ctypes.byref(neg_tol), n=0x80000000),
              with_(prm=ctypes.byref(neg_tol), boxes=None)):
        assert call(a) == P.ERR_ARG and untouched()
    # UNSUPPORTED: too many regions, too many points -- before any label is read (the label array has 65 entries)
    assert call(with_(K=0x01000000)) == P.ERR_UNSUPPORTED and untouched()
    assert call(with_(n=0x80000000)) == P.ERR_UNSUPPORTED and untouched()
    assert call(with_(K=0x00FFFFFF + 1, lab=bad_lab.ctypes.data)) == P.ERR_UNSUPPORTED and untouched()
    # ARG: a label out of range, on a finite point and on a non-finite one only
    assert call(with_(lab=bad_lab.ctypes.data)) == P.ERR_ARG and untouched()
    nf = pts.copy(); nf[3, 1] = np.nan
    assert call(with_(pts=nf.ctypes.data, lab=bad_lab.ctypes.data)) == P.ERR_ARG and untouched()
    far = lab.copy(); far[-1] = 0xFFFFFFFE
    assert call(with_(lab=far.ctypes.data)) == P.ERR_ARG and untouched()
    # what is allowed: NULL params (the defaults), NULL boxes, NULL result, +inf and zero tolerances, NULL points with n == 0, NULL rows without regions
    assert call(with_(prm=None)) == 0 and res.n_regions == K
    want = C.ref_cloud(P, pts, lab, K)
    C.assert_rows_equal(rows, want[1]); B.assert_rows_equal(P, boxes, want[2]); assert res.as_dict() == want[3]
    for a in (with_(boxes=None), with_(res=None), with_(prm=ctypes.byref(P.CloudParams(float("inf"), 0))), with_(prm=ctypes.byref(P.CloudParams(0.0, 0))),
              with_(prm=ctypes.byref(P.CloudParams(-0.0, 0))), with_(pts=None, n=0)):
        assert call(a) == 0
    none = np.full(len(lab), NO, np.uint32)
    assert call(with_(lab=none.ctypes.data, K=0, rows=None, boxes=None)) == 0 and res.as_dict() == dict(n_regions=0, n_nonempty=0, n_labelled=0, n_clamped=0, n_inliers=0)
    assert call(with_(K=0, rows=None, boxes=None)) == P.ERR_ARG      # any label but F3DS_NO_LABEL is out of range then


# ---- 5. the host code under the sanitizers: a stand-alone executable, no Python in the process -----------------------------------------------------------------
def test_host_code_runs_clean_under_the_sanitizers(tmp_path):
    import os, shutil, subprocess
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cloud_regions_host_main.cpp"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cloud_regions_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-static-libasan", "-static-libubsan", "-o", exe,      # (the runtimes inside the executable: nothing depends on the order libraries load in)
                            os.path.join(root, "tests", "cloud_regions_host_main.cpp"),
                            os.path.join(root, "fast-3d-pointcloud-segmentation_amd", "csrc", "f3ds_host.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and ran.stdout.strip() == "cloud_regions_host: ok" and not ran.stderr.strip(), (ran.returncode, ran.stdout[-500:], ran.stderr[-2000:])
