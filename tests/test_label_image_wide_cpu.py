"""The label-image calls at frames wider than a workgroup (tests/label_image_wide_common.py), without a GPU: the CENSUS -- the kernels' constants as the
library itself names them (P.constant), every case reaching the classes of control flow it is for, every class populated -- and the `_host` form of every call against
its Python reference at every case, bit for bit: f3ds_region_table_host, _contacts_host, _shapes_host, _boxes_host, _components_host,
f3ds_region_components_tiled (the kernels' union-find steps, sequentially) at tile sizes 64 x 16 and 3 x 5, and the tracker's update composed from
f3ds_deproject, f3ds_track_reproject and f3ds_track_assign as tests/test_track_cpu.py composes it.  This is what shows that the references are right at the new
shapes before a GPU sees them; tests/test_label_image_wide_gpu.py compares the device with the same cached references."""

import numpy as np
import pytest

import label_image_wide_common as W
import region_boxes_common as B
import region_components_common as C
import region_contacts_common as CT
import region_shapes_common as S
import region_table_common as R
from label_image_wide_common import INF, NO
from track_common import f32

IDS = [c.id for c in W.CASES]


# ---- the census -----------------------------------------------------------------------------------------------------------------------------------------------

def test_the_kernels_constants_are_the_census_constants(P):
    got = [(name, P.constant(name), want) for name, want in W.KERNEL_CONSTANTS.items()]
    assert len(got) == 18
    for name, have, want in got:
        assert have == want, "%s is %r, the census assumes %r" % (name, have, want)
    # the remainder of the accumulator sets and the carry of the span walk: the classes that sit on either side of them all have cases
    sides = [cl for classes in W.OPERATOR_CLASSES.values() for cl in classes]
    assert len(sides) == 6 and all(any(cl in c.classes for c in W.CASES) for cl in sides)
    assert W.rgt_copies(1) == 32 and W.rgt_copies(64) == 32 and W.rgt_copies(65) == 31 and W.rgt_copies(2049) == 1 and W.rgt_copies(0) == 32


def test_the_launch_arithmetic_at_the_new_sizes_and_at_the_earlier_ones():
    assert W.accum_grid(160 * 120, W.LI_TRIPS) == 19                                    # the widest frame of the family's other tests: never past 32 sets
    assert W.accum_grid(255 * 9, W.LI_TRIPS) == W.accum_grid(257 * 9, W.LI_TRIPS) == 3
    assert W.accum_grid(321 * 113, W.LI_TRIPS) == 36 and W.accum_grid(640 * 61, W.LI_TRIPS) == 39
    assert W.accum_grid(321 * 113, W.LI_TRIPS, 1) == 1 and W.span_of(321 * 113, 1) // W.BLOCK == 142      # one workgroup: 142 trips
    assert W.tiles_of(321, 113) == (6, 8) and W.tiles_of(640, 61) == (10, 4) and W.tiles_of(257, 9) == (5, 1) and W.tiles_of(97, 61) == (2, 4)
    assert [W.step_of(w) for w in (255, 256, 257, 128, 512, 321, 640)] == [(1, 1), (1, 0), (0, 256), (2, 0), (0, 256), (0, 256), (0, 256)]
    assert all(W.step_of(w)[0] >= 1 for w in (97, 67, 3, 1, 40, 33, 160))                # what the family's other tests run: sv >= 1 always


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_a_case_reaches_the_classes_it_is_for(P, case):
    c = W.census(P, case)
    assert set(case.classes) <= c["reached"], (case.id, sorted(set(case.classes) - c["reached"]), c)
    assert set(case.classes) <= set(W.CLASSES)
    fr = W.frame(P, case)
    assert fr["K"] <= 0x00FFFFFF and case.n <= 40000                                     # LI_MAX_REGIONS; the references stay near a second
    if "wrap32" in case.classes:
        assert c["workgroups"] > c["copies"] == 32 and fr["K"] <= 64
    if "lds_overflow" in case.classes:
        assert c["labels_per_span"] > W.LI_SLOTS and c["pairs_per_span"] > W.RGC_SLOTS
    if "spiral_seams" in case.classes:
        assert c["seam_links"] >= c["tiles_x"] * c["tiles_y"] >= 40


def test_every_class_is_populated_and_every_shape_and_scene_is_there():
    for name in W.CLASSES:
        assert any(name in c.classes for c in W.CASES), name
    assert len(W.CASES) == len(W.SHAPES) * len(W.SCENES) == 77 and len(set(IDS)) == 77
    by = lambda name: sorted(set(c.width for c in W.CASES if name in c.classes))
    assert by("sv0") == [257, 321, 512, 640] and by("su0_sv1") == [256] and by("su0_sv2") == [128] and by("below_block") == [255]
    assert by("two_blocks") == [512, 640] and by("wrap32") == [321, 640] and by("tiles5_partial") == [257, 321] and by("spiral_seams") == [321, 640]
    assert by("lds_overflow") == by("pairs_overflow") == sorted(s[0] for s in W.SHAPES)
    assert any("wrap32" in c.classes and c.scene == "table2" for c in W.CASES)           # every flush of every workgroup onto one region, 32 sets
    for w in W.ALL_COLORS_AT:
        assert all(len(c.colors) == 4 for c in W.CASES if c.width == w)
    assert set(k for c in W.CASES for k in c.colors) == set(R.COLORS)
    # only scene 3 is shortened, and the full frames are there
    assert all((c.width, c.height) in [s[:2] for s in W.SHAPES] for c in W.CASES if c.scene != "table3")
    assert W.BAD_LABEL_CASE.width == 640 and W.BAD_LABEL_CASE.height == 61


# ---- the host functions against the references --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_table_host_equals_the_reference(P, case):
    fr = W.frame(P, case)
    for ck in case.colors:
        wrc, wrows, wres = W.reference(P, case, "table", ck)
        rows, res = P.region_table_host(W.depth_view(case, fr), fr["labels"], fr["K"], R.with_color(P, fr["fmt"], ck), W.color_view(case, fr, ck))
        assert wrc == 0
        R.assert_rows_equal(P, rows, wrows, "%s %s" % (case.id, ck))
        assert res.as_dict() == wres, (res.as_dict(), wres)
    if case.scene == "table8":
        assert wres["n_clamped"] > 0
    if case.scene == "table3":
        assert wres["n_nonempty"] > 10 * W.LI_SLOTS


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_shapes_and_boxes_host_equal_the_reference(P, case):
    fr = W.frame(P, case)
    wrc, wrows, wshapes, wres = W.reference(P, case, "boxes")
    assert wrc == 0
    depth = W.depth_view(case, fr)
    rows, res = P.region_shapes_host(depth, fr["labels"], fr["K"], fr["fmt"])
    S.assert_rows_equal(P, rows, wshapes, case.id)
    assert res.as_dict() == W.shapes_result(wres)
    rows, shapes, res = P.region_boxes_host(depth, fr["labels"], fr["K"], fr["fmt"], B.TOL, want_shapes=True)
    B.assert_rows_equal(P, rows, wrows, case.id)
    S.assert_rows_equal(P, shapes, wshapes, case.id)
    assert res.as_dict() == wres, (res.as_dict(), wres)


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_contacts_host_equals_the_reference(P, case):
    fr = W.frame(P, case)
    for tol in W.CONTACT_TOLS:
        wrc, wrows, wres = W.reference(P, case, "contacts", tol)
        rows, res = P.region_contacts_host(W.depth_view(case, fr), fr["labels"], fr["K"], fr["fmt"], tol)
        assert wrc == 0
        CT.assert_rows_equal(rows, wrows, "%s %s" % (case.id, tol))
        assert res.as_dict() == wres, (res.as_dict(), wres)
        if tol > 1:
            assert wres["n_close"] == wres["n_pairs"]
    if case.scene == "table3":
        assert len(wrows) > 10 * W.RGC_SLOTS
    with pytest.raises(P.F3dsError) as e:      # the contacts take no infinite tolerance (include/f3ds.h); the components do
        P.region_contacts_host(W.depth_view(case, fr), fr["labels"], fr["K"], fr["fmt"], INF)
    assert e.value.code == P.ERR_ARG


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_components_host_and_the_tiled_run_equal_the_reference(P, case):
    fr = W.frame(P, case)
    for tol in (0.05, INF):
        for minpix in case.min_pixels:
            wrc, wimage, wrows, wres = W.reference(P, case, "components", tol, minpix)
            assert wrc == 0
            image, rows, res = P.region_components_host(W.depth_view(case, fr), fr["labels"], fr["K"], fr["fmt"], tol, minpix)
            C.assert_same(image, rows, wimage, wrows, "%s %s %d" % (case.id, tol, minpix))
            assert res.as_dict() == wres, (res.as_dict(), wres)
            for tile in ((W.CC_TILE_W, W.CC_TILE_H), (3, 5)):
                rc, image, rows, res = W.c_components_tiled(P, case, fr, tol, minpix, tile)
                assert rc == 0
                C.assert_same(image, rows, wimage, wrows, "%s %s %d tile %s" % (case.id, tol, minpix, tile))
                assert res.as_dict() == wres, (res.as_dict(), wres)
    if case.scene == "speckles":
        assert wres["n_dropped"] > 0 and wres["n_components"] > 0                        # (min_pixels 3: the last one of the loop)
    if case.scene in ("spiral", "comb_right", "comb_bottom") and case.height > 5:
        assert W.reference(P, case, "components", INF, 1)[3]["n_components"] <= 2        # the seams join what the tiles see apart


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_the_tracker_s_host_functions_compose_to_the_reference(P, case):
    fr = W.frame(P, case)
    fmt, K = fr["fmt"], fr["K"]
    want = W.reference(P, case, "track")
    prm = P.default_track_params()
    pts = P.deproject(fmt.copy(), fr["depth"], np.zeros((case.height, case.width, 3), np.uint8))
    valid = ~np.isnan(pts[:, 2])
    slot = zprev = None; prev_id = np.zeros(0, np.uint32); nxt = 0
    for (labels, reset), (wrc, wimg, wids, wres) in zip(W.track_frames(fr), want):
        assert wrc == 0
        if reset:
            slot = zprev = None; prev_id = np.zeros(0, np.uint32)
        lab = labels.reshape(-1)
        labelled = valid & (lab != NO)
        size = np.bincount(lab[labelled], minlength=K)
        entries = np.zeros((0, 3), np.int64)
        if slot is not None:
            pixel, zp = P.track_reproject(fmt, pts, None)
            q = np.where(pixel >= 0, pixel, 0)
            with np.errstate(all="ignore"):
                vote = labelled & (pixel >= 0) & (slot[q] != NO) & (np.abs(zp - zprev[q]) <= f32(prm.depth_tol) * zp)
            if vote.any():
                u, c = np.unique(np.stack([lab[vote].astype(np.int64), slot[q][vote].astype(np.int64)], axis=1), axis=0, return_counts=True)
                entries = np.concatenate([u, c[:, None]], axis=1)
        ids, nxt, res = P.track_assign(size, entries, prev_id, nxt, prm)
        assert np.array_equal(ids, wids), case.id
        got = res.as_dict(); got["first_frame"] = 1 if slot is None else 0
        assert got == wres, (case.id, got, wres)
        out = np.full(case.n, NO, np.uint32); has = lab != NO
        out[has] = ids[lab[has]]
        assert np.array_equal(out, wimg)
        slot, zprev, prev_id = np.where(labelled, lab, np.uint32(NO)), pts[:, 2].copy(), ids
    # the second and third frames match the first's regions one to one wherever a region has the votes
    assert want[1][3]["n_matched"] == want[2][3]["n_matched"] and want[3][3]["first_frame"] == 1 and want[3][3]["n_matched"] == 0
