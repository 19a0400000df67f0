"""f3ds -- MI355X-native supervoxel + hierarchical-merge segmenter (host-side binding).

Thin ctypes layer over the C-ABI in ``include/f3ds.h`` (``libf3ds.so``, hand-written HIP for
gfx950).  The classes mirror the reference's interface for this path:

* :class:`Clustering`   -- ``/root/reference/include/supervoxel_clustering/clustering.h:84-212``
  (same setter names, same exceptions: ``logic_error`` -> :class:`LogicError`,
  ``invalid_argument`` -> ``ValueError``), fed by :class:`SupervoxelClustering`, the stand-in
  for ``pcl::SupervoxelClustering<PointXYZRGBA>`` as ``main()`` drives it
  (``/root/reference/src/supervoxel_clustering.cpp:348-367``).
* :func:`segment`       -- the whole frame in one call (what ``main()`` does between ``:313``
  and ``:449``).

There is no CPU fallback: constructing a :class:`Context` without a GPU, or with the shared
library missing, raises.  PyTorch is not required; device pointers (e.g. ``tensor.data_ptr()``)
can be passed with ``on_device=True``.
"""
import ctypes
import os
import struct

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
def _dev_env(name):
    """A development switch of the environment: only read while F3DS_DEV is set (csrc/f3ds_dev.h; the library applies the same gate)."""
    return os.environ.get(name) if os.environ.get("F3DS_DEV", "0") not in ("", "0") else None


LIB_PATH = _dev_env("F3DS_LIB") or os.path.join(_HERE, "libf3ds.so")       # F3DS_LIB (with F3DS_DEV=1): A/B builds during development

NO_LABEL = 0xFFFFFFFF
LAB_CIEDE00, RGB_EUCL = 0, 1
NORMALS_DIFF, CONVEX_NORMALS_DIFF = 0, 1
MANUAL_LAMBDA, ADAPTIVE_LAMBDA, EQUALIZATION = 0, 1, 2
DEPTH_U16, DEPTH_F32 = 0, 1
COLOR_RGB8, COLOR_RGBA8, COLOR_PACKED = 0, 1, 2

# debug selectors (include/f3ds.h)
DBG = dict(GRID=0, VOXEL_KEYS=1, VOXEL_COUNT=2, VOXEL_XYZ=3, VOXEL_RGB=4, VOXEL_NORMAL=5, VOXEL_NEIGHBORS=6,
           POINT_VOXEL=7, SEED_ORIG=8, SEED_KEPT=9, VOXEL_SVLABEL=10, VOXEL_DIST=11, SV_LABELS=12, SV_CENTROID=13,
           EDGES=14, EDGE_DELTAS=15, EDGE_WEIGHTS=16, MERGES=17, VOXEL_REGION=18, SV_REGION=19)
# ... and the selectors of diagnostics (a few words about the last call, not an array of the frame): Context.merge_layout() etc.
DBG_INFO = dict(MERGE_LAYOUT=20, TILE_LIST_LEN=21, SWEEP_STATS=22, STAGE0_PATH=23, LAUNCH_SHAPE=24)
DBG_CLOUD_PATH = 25      # F3DS_DBG_CLOUD_PATH (include/f3ds.h): a selector of the region family, outside the enum of the frame's hooks
DBG_DTYPE = dict(GRID=np.float64, VOXEL_KEYS=np.uint32, VOXEL_COUNT=np.uint32, VOXEL_XYZ=np.float32, VOXEL_RGB=np.float32,
                 VOXEL_NORMAL=np.float32, VOXEL_NEIGHBORS=np.int32, POINT_VOXEL=np.int32, SEED_ORIG=np.int32, SEED_KEPT=np.int32,
                 VOXEL_SVLABEL=np.uint32, VOXEL_DIST=np.float32, SV_LABELS=np.uint32, SV_CENTROID=np.float32, EDGES=np.uint32,
                 EDGE_DELTAS=np.float32, EDGE_WEIGHTS=np.float32, MERGES=np.uint32, VOXEL_REGION=np.uint32, SV_REGION=np.uint32)


class F3dsError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("f3ds error %d: %s" % (code, text))
        self.code = code


class LogicError(F3dsError):
    """std::logic_error of the reference (clustering.cpp:576,591,671)."""


class Params(ctypes.Structure):
    _fields_ = [("voxel_res", ctypes.c_float), ("seed_res", ctypes.c_float), ("w_color", ctypes.c_float),
                ("w_spatial", ctypes.c_float), ("w_normal", ctypes.c_float), ("use_transform", ctypes.c_int32),
                ("color_metric", ctypes.c_int32), ("geom_metric", ctypes.c_int32), ("merging", ctypes.c_int32),
                ("lambda_", ctypes.c_float), ("bins", ctypes.c_int32), ("threshold", ctypes.c_float),
                ("leaf_order", ctypes.c_int32), ("fold_negative_z", ctypes.c_int32)]

    def copy(self):
        p = Params()
        ctypes.memmove(ctypes.byref(p), ctypes.byref(self), ctypes.sizeof(Params))
        return p


class Result(ctypes.Structure):
    _fields_ = [("n_points", ctypes.c_uint64), ("n_finite", ctypes.c_uint64), ("n_voxels", ctypes.c_uint32),
                ("octree_depth", ctypes.c_uint32), ("n_seed_cells", ctypes.c_uint32), ("n_seeds", ctypes.c_uint32),
                ("n_supervoxels", ctypes.c_uint32), ("n_edges", ctypes.c_uint32), ("n_merges", ctypes.c_uint32),
                ("n_regions", ctypes.c_uint32), ("sweeps", ctypes.c_uint32), ("lambda_", ctypes.c_float),
                ("ms_total", ctypes.c_float), ("ms_stage", ctypes.c_float * 8)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "ms_stage"}
        d["ms_stage"] = list(self.ms_stage)
        return d


class RgbdFormat(ctypes.Structure):
    """f3ds_rgbd_format (include/f3ds.h): size, element types and pinhole intrinsics of a depth + colour image pair.  Pitches are bytes per
    image row, 0 = tightly packed; the wrappers that take numpy images fill them in from the arrays' row strides."""
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("depth_type", ctypes.c_int32), ("depth_scale", ctypes.c_float),
                ("color_format", ctypes.c_int32), ("depth_pitch", ctypes.c_uint32), ("color_pitch", ctypes.c_uint32),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float)]

    def copy(self):
        f = RgbdFormat()
        ctypes.memmove(ctypes.byref(f), ctypes.byref(self), ctypes.sizeof(RgbdFormat))
        return f


class TrackParams(ctypes.Structure):
    """f3ds_track_params (include/f3ds.h): when a region takes over a previous id."""
    _fields_ = [("min_votes", ctypes.c_uint32), ("min_permille", ctypes.c_uint32), ("depth_tol", ctypes.c_float)]


class TrackResult(ctypes.Structure):
    """f3ds_track_result (include/f3ds.h): the counts of one tracker update."""
    _fields_ = [(k, ctypes.c_uint32) for k in ("n_regions", "n_nonempty", "n_matched", "n_new", "n_retired", "n_entries", "next_id", "first_frame")] + \
               [("n_labelled", ctypes.c_uint64), ("n_votes", ctypes.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class RegionRow(ctypes.Structure):
    """f3ds_region_row (include/f3ds.h): one region of a label image over an RGB-D frame, 72 bytes."""
    _fields_ = [(k, ctypes.c_uint32) for k in ("n_pixels", "first_pixel", "u_min", "v_min", "u_max", "v_max")] + \
               [(k, ctypes.c_float * 3) for k in ("lo", "hi", "centroid", "mean_rgb")]


class RegionTableResult(ctypes.Structure):
    """f3ds_region_table_result (include/f3ds.h): the counts of one region table."""
    _fields_ = [("n_regions", ctypes.c_uint32), ("n_nonempty", ctypes.c_uint32), ("n_labelled", ctypes.c_uint64), ("n_clamped", ctypes.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# the same 72 bytes as a numpy structured dtype: what region_table_host and Context.region_table return their rows in
REGION_ROW_DTYPE = np.dtype([(k, np.uint32) for k in ("n_pixels", "first_pixel", "u_min", "v_min", "u_max", "v_max")] +
                            [(k, np.float32, (3,)) for k in ("lo", "hi", "centroid", "mean_rgb")])
assert REGION_ROW_DTYPE.itemsize == ctypes.sizeof(RegionRow) == 72


class RegionContact(ctypes.Structure):
    """f3ds_region_contact (include/f3ds.h): one pair of regions of a label image that touch, 32 bytes."""
    _fields_ = [(k, ctypes.c_uint32) for k in ("a", "b", "n_pairs", "n_close", "n_a_front", "n_horizontal", "first_pixel")] + [("mean_gap", ctypes.c_float)]


class RegionContactsResult(ctypes.Structure):
    """f3ds_region_contacts_result (include/f3ds.h): the counts of one call for the region contacts."""
    _fields_ = [("n_regions", ctypes.c_uint32), ("n_contacts", ctypes.c_uint32), ("n_pairs", ctypes.c_uint64), ("n_close", ctypes.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# the same 32 bytes as a numpy structured dtype: what region_contacts_host and Context.region_contacts return their rows in
REGION_CONTACT_DTYPE = np.dtype([(k, np.uint32) for k in ("a", "b", "n_pairs", "n_close", "n_a_front", "n_horizontal", "first_pixel")] + [("mean_gap", np.float32)])
assert REGION_CONTACT_DTYPE.itemsize == ctypes.sizeof(RegionContact) == 32


class RegionShape(ctypes.Structure):
    """f3ds_region_shape (include/f3ds.h): covariance, eigenvalues, plane and long axis of one region of a label image, 84 bytes."""
    _fields_ = [("n_pixels", ctypes.c_uint32), ("centroid", ctypes.c_float * 3), ("cov", ctypes.c_float * 6), ("eigenvalue", ctypes.c_float * 3),
                ("normal", ctypes.c_float * 3), ("axis", ctypes.c_float * 3), ("plane_d", ctypes.c_float), ("curvature", ctypes.c_float)]


class RegionShapesResult(ctypes.Structure):
    """f3ds_region_shapes_result (include/f3ds.h): the counts of one call for the region shapes."""
    _fields_ = [("n_regions", ctypes.c_uint32), ("n_nonempty", ctypes.c_uint32), ("n_labelled", ctypes.c_uint64), ("n_clamped", ctypes.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# the same 84 bytes as a numpy structured dtype: what region_shapes_host and Context.region_shapes return their rows in
REGION_SHAPE_DTYPE = np.dtype([("n_pixels", np.uint32), ("centroid", np.float32, (3,)), ("cov", np.float32, (6,)), ("eigenvalue", np.float32, (3,)),
                               ("normal", np.float32, (3,)), ("axis", np.float32, (3,)), ("plane_d", np.float32), ("curvature", np.float32)])
assert REGION_SHAPE_DTYPE.itemsize == ctypes.sizeof(RegionShape) == 84


class RegionBox(ctypes.Structure):
    """f3ds_region_box (include/f3ds.h): the box of one region of a label image along the region's own axes and its plane residuals, 96 bytes."""
    _fields_ = [("n_pixels", ctypes.c_uint32), ("n_inliers", ctypes.c_uint32)] + \
               [(k, ctypes.c_float * 3) for k in ("center", "axis_n", "axis_m", "axis_l", "lo", "hi", "half")] + [("mean_abs_residual", ctypes.c_float)]


class RegionBoxesResult(ctypes.Structure):
    """f3ds_region_boxes_result (include/f3ds.h): the counts of one call for the region boxes."""
    _fields_ = [("n_regions", ctypes.c_uint32), ("n_nonempty", ctypes.c_uint32), ("n_labelled", ctypes.c_uint64), ("n_clamped", ctypes.c_uint64),
                ("n_inliers", ctypes.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# the same 96 bytes as a numpy structured dtype: what region_boxes_host and Context.region_boxes return their rows in
REGION_BOX_DTYPE = np.dtype([("n_pixels", np.uint32), ("n_inliers", np.uint32)] +
                            [(k, np.float32, (3,)) for k in ("center", "axis_n", "axis_m", "axis_l", "lo", "hi", "half")] + [("mean_abs_residual", np.float32)])
assert REGION_BOX_DTYPE.itemsize == ctypes.sizeof(RegionBox) == 96


class CloudParams(ctypes.Structure):
    """f3ds_cloud_params (include/f3ds.h): the boxes' inlier distance and the segmenter's fold of negative z."""
    _fields_ = [("plane_tol", ctypes.c_float), ("fold_negative_z", ctypes.c_int32)]


class CloudRegion(ctypes.Structure):
    """f3ds_cloud_region (include/f3ds.h): one region of a labelled point cloud -- the table's and the shapes' fields in one row, 128 bytes."""
    _fields_ = [("n_points", ctypes.c_uint32), ("first_point", ctypes.c_uint32)] + \
               [(k, ctypes.c_float * 3) for k in ("lo", "hi", "centroid", "mean_rgb")] + [("cov", ctypes.c_float * 6)] + \
               [(k, ctypes.c_float * 3) for k in ("eigenvalue", "normal", "axis")] + [("plane_d", ctypes.c_float), ("curvature", ctypes.c_float), ("reserved", ctypes.c_uint32)]


class CloudRegionsResult(ctypes.Structure):
    """f3ds_cloud_regions_result (include/f3ds.h): the counts of one call for the region rows of a cloud."""
    _fields_ = [("n_regions", ctypes.c_uint32), ("n_nonempty", ctypes.c_uint32), ("n_labelled", ctypes.c_uint64), ("n_clamped", ctypes.c_uint64),
                ("n_inliers", ctypes.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# the same 128 bytes as a numpy structured dtype: what cloud_regions_host and Context.cloud_regions return their rows in
CLOUD_REGION_DTYPE = np.dtype([("n_points", np.uint32), ("first_point", np.uint32)] + [(k, np.float32, (3,)) for k in ("lo", "hi", "centroid", "mean_rgb")] +
                              [("cov", np.float32, (6,))] + [(k, np.float32, (3,)) for k in ("eigenvalue", "normal", "axis")] +
                              [("plane_d", np.float32), ("curvature", np.float32), ("reserved", np.uint32)])
assert CLOUD_REGION_DTYPE.itemsize == ctypes.sizeof(CloudRegion) == 128


class JointParams(ctypes.Structure):
    """f3ds_joint_params (include/f3ds.h): the contacts' depth tolerance, and the plane distance and the cosine below which two regions count as coplanar."""
    _fields_ = [("depth_tol", ctypes.c_float), ("plane_tol", ctypes.c_float), ("cos_coplanar", ctypes.c_float)]


class RegionJoint(ctypes.Structure):
    """f3ds_region_joint (include/f3ds.h): the border of two touching regions in space and the relation of their planes, 80 bytes."""
    _fields_ = [(k, ctypes.c_uint32) for k in ("a", "b", "n_pairs", "n_close")] + [(k, ctypes.c_float * 3) for k in ("centroid", "direction", "spread")] + \
               [(k, ctypes.c_float) for k in ("cos_angle", "delta_g", "h_ab", "h_ba", "e_a", "e_b")] + [("kind", ctypes.c_uint32)]


class RegionJointsResult(ctypes.Structure):
    """f3ds_region_joints_result (include/f3ds.h): the counts of one call for the region joints."""
    _fields_ = [(k, ctypes.c_uint32) for k in ("n_regions", "n_joints", "n_surface", "reserved")] + [("n_pairs", ctypes.c_uint64), ("n_close", ctypes.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# the same 80 bytes as a numpy structured dtype: what region_joints_host and Context.region_joints return their rows in
REGION_JOINT_DTYPE = np.dtype([(k, np.uint32) for k in ("a", "b", "n_pairs", "n_close")] + [(k, np.float32, (3,)) for k in ("centroid", "direction", "spread")] +
                              [(k, np.float32) for k in ("cos_angle", "delta_g", "h_ab", "h_ba", "e_a", "e_b")] + [("kind", np.uint32)])
assert REGION_JOINT_DTYPE.itemsize == ctypes.sizeof(RegionJoint) == 80
JOINT_OCCLUSION, JOINT_COPLANAR, JOINT_CONVEX, JOINT_CONCAVE, JOINT_KIND_MASK, JOINT_REF_CONVEX = 0, 1, 2, 3, 0xFF, 0x100      # the values and the flag of `kind`


class ComponentParams(ctypes.Structure):
    """f3ds_component_params (include/f3ds.h): the depth tolerance of a link and the smallest component that is kept."""
    _fields_ = [("depth_tol", ctypes.c_float), ("min_pixels", ctypes.c_uint32)]


class RegionComponent(ctypes.Structure):
    """f3ds_region_component (include/f3ds.h): one connected component of a label image, 12 bytes."""
    _fields_ = [(k, ctypes.c_uint32) for k in ("region", "first_pixel", "n_pixels")]


class RegionComponentsResult(ctypes.Structure):
    """f3ds_region_components_result (include/f3ds.h): the counts of one call for the region components."""
    _fields_ = [(k, ctypes.c_uint32) for k in ("n_regions", "n_components", "n_dropped", "reserved")] + [("n_labelled", ctypes.c_uint64), ("n_kept", ctypes.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# the same 12 bytes as a numpy structured dtype: what region_components_host and Context.region_components return their rows in
REGION_COMPONENT_DTYPE = np.dtype([(k, np.uint32) for k in ("region", "first_pixel", "n_pixels")])
assert REGION_COMPONENT_DTYPE.itemsize == ctypes.sizeof(RegionComponent) == 12


class SupervoxelSet(ctypes.Structure):
    """f3ds_supervoxel_set (include/f3ds.h): the supervoxel_clusters map of the reference as plain arrays."""
    _fields_ = [("n_supervoxels", ctypes.c_uint32), ("label", ctypes.c_void_p), ("voxel_offset", ctypes.c_void_p), ("voxel_xyz", ctypes.c_void_p),
                ("voxel_rgba", ctypes.c_void_p), ("centroid_xyz", ctypes.c_void_p), ("normal", ctypes.c_void_p)]


_lib = None


class Performance(ctypes.Structure):
    """performanceSet (include/supervoxel_clustering/testing.h:40-48)."""
    _fields_ = [(k, ctypes.c_float) for k in ("voi", "precision", "recall", "fscore", "wov", "fpr", "fnr")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def load_library(path=None):
    """Load libf3ds.so (built by ``__graft_entry__.build()`` / ``make -C csrc``).  Raises if missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ImportError("libf3ds.so not found at %s -- build it first (python -c 'import __graft_entry__ as g; g.build()'); "
                          "this package has no CPU fallback" % p)
    lib = ctypes.CDLL(p)
    vp, sz, u32p = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)
    lib.f3ds_default_params.argtypes = [ctypes.POINTER(Params)]; lib.f3ds_default_params.restype = None
    lib.f3ds_version.restype = ctypes.c_int
    if hasattr(lib, "f3ds_version_string"):      # (F3DS_LIB may point at an older build during A/B runs)
        lib.f3ds_version_string.restype = ctypes.c_char_p
    lib.f3ds_strerror.argtypes = [ctypes.c_int]; lib.f3ds_strerror.restype = ctypes.c_char_p
    lib.f3ds_last_hip_error.restype = ctypes.c_char_p
    lib.f3ds_device_count.restype = ctypes.c_int
    lib.f3ds_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]; lib.f3ds_create.restype = ctypes.c_int
    lib.f3ds_destroy.argtypes = [vp]; lib.f3ds_destroy.restype = None
    lib.f3ds_set_stream.argtypes = [vp, vp]; lib.f3ds_set_stream.restype = ctypes.c_int
    lib.f3ds_segment.argtypes = [vp, vp, sz, ctypes.c_int, ctypes.POINTER(Params), vp, ctypes.c_int, ctypes.POINTER(Result)]
    lib.f3ds_segment.restype = ctypes.c_int
    lib.f3ds_segment_batch.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.c_int, ctypes.POINTER(Params),
                                       ctypes.POINTER(vp), ctypes.c_int, ctypes.POINTER(Result)]
    lib.f3ds_segment_batch.restype = ctypes.c_int
    if hasattr(lib, "f3ds_segment_rgbd"):      # (RGB-D frames; F3DS_LIB may point at an older build during A/B runs)
        fp = ctypes.POINTER(RgbdFormat)
        lib.f3ds_deproject.argtypes = [fp, vp, vp, vp]; lib.f3ds_deproject.restype = ctypes.c_int
        lib.f3ds_segment_rgbd.argtypes = [vp, fp, vp, vp, ctypes.c_int, ctypes.POINTER(Params), vp, ctypes.c_int, ctypes.POINTER(Result)]
        lib.f3ds_segment_rgbd.restype = ctypes.c_int
        lib.f3ds_segment_rgbd_batch.argtypes = [ctypes.POINTER(vp), ctypes.c_int, fp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.c_int, ctypes.POINTER(Params),
                                                ctypes.POINTER(vp), ctypes.c_int, ctypes.POINTER(Result)]
        lib.f3ds_segment_rgbd_batch.restype = ctypes.c_int
        lib.f3ds_get_points.argtypes = [vp, vp, sz, ctypes.c_int, ctypes.POINTER(sz)]; lib.f3ds_get_points.restype = ctypes.c_int
        lib.f3ds_stream_submit_rgbd.argtypes = [vp, fp, vp, vp, ctypes.POINTER(Params), ctypes.c_uint64]; lib.f3ds_stream_submit_rgbd.restype = ctypes.c_int
    if hasattr(lib, "f3ds_tracker_update"):
        tpp, trp = ctypes.POINTER(TrackParams), ctypes.POINTER(TrackResult)
        lib.f3ds_default_track_params.argtypes = [tpp]; lib.f3ds_default_track_params.restype = None
        lib.f3ds_tracker_create.argtypes = [ctypes.c_int, tpp, ctypes.POINTER(vp)]; lib.f3ds_tracker_create.restype = ctypes.c_int
        lib.f3ds_tracker_destroy.argtypes = [vp]; lib.f3ds_tracker_destroy.restype = None
        lib.f3ds_tracker_set_stream.argtypes = [vp, vp]; lib.f3ds_tracker_set_stream.restype = ctypes.c_int
        lib.f3ds_tracker_reset.argtypes = [vp]; lib.f3ds_tracker_reset.restype = ctypes.c_int
        lib.f3ds_tracker_update.argtypes = [vp, ctypes.POINTER(RgbdFormat), vp, vp, ctypes.c_uint32, ctypes.c_int, vp, vp, ctypes.c_int, trp]
        lib.f3ds_tracker_update.restype = ctypes.c_int
        lib.f3ds_tracker_get_ids.argtypes = [vp, vp, sz, ctypes.POINTER(sz)]; lib.f3ds_tracker_get_ids.restype = ctypes.c_int
        lib.f3ds_track_reproject.argtypes = [ctypes.POINTER(RgbdFormat), vp, vp, sz, vp, vp]; lib.f3ds_track_reproject.restype = ctypes.c_int
        lib.f3ds_track_assign.argtypes = [tpp, vp, ctypes.c_uint32, vp, sz, vp, ctypes.c_uint32, u32p, vp, trp]; lib.f3ds_track_assign.restype = ctypes.c_int
    if hasattr(lib, "f3ds_region_table"):
        rtp = ctypes.POINTER(RegionTableResult)
        lib.f3ds_region_table_host.argtypes = [ctypes.POINTER(RgbdFormat), vp, vp, vp, ctypes.c_uint32, vp, rtp]; lib.f3ds_region_table_host.restype = ctypes.c_int
        lib.f3ds_region_table.argtypes = [vp, ctypes.POINTER(RgbdFormat), vp, vp, vp, ctypes.c_uint32, ctypes.c_int, vp, ctypes.c_int, rtp]
        lib.f3ds_region_table.restype = ctypes.c_int
    if hasattr(lib, "f3ds_region_contacts"):
        rcp = ctypes.POINTER(RegionContactsResult)
        lib.f3ds_region_contacts_host.argtypes = [ctypes.POINTER(RgbdFormat), vp, vp, ctypes.c_uint32, ctypes.c_float, vp, sz, ctypes.POINTER(sz), rcp]
        lib.f3ds_region_contacts_host.restype = ctypes.c_int
        lib.f3ds_region_contacts.argtypes = [vp, ctypes.POINTER(RgbdFormat), vp, vp, ctypes.c_uint32, ctypes.c_float, ctypes.c_int, vp, sz, ctypes.c_int, ctypes.POINTER(sz), rcp]
        lib.f3ds_region_contacts.restype = ctypes.c_int
    if hasattr(lib, "f3ds_region_shapes"):
        rsp = ctypes.POINTER(RegionShapesResult)
        lib.f3ds_region_shapes_host.argtypes = [ctypes.POINTER(RgbdFormat), vp, vp, ctypes.c_uint32, vp, rsp]; lib.f3ds_region_shapes_host.restype = ctypes.c_int
        lib.f3ds_region_shapes.argtypes = [vp, ctypes.POINTER(RgbdFormat), vp, vp, ctypes.c_uint32, ctypes.c_int, vp, ctypes.c_int, rsp]
        lib.f3ds_region_shapes.restype = ctypes.c_int
    if hasattr(lib, "f3ds_region_boxes"):
        rbp = ctypes.POINTER(RegionBoxesResult)
        lib.f3ds_region_boxes_host.argtypes = [ctypes.POINTER(RgbdFormat), vp, vp, ctypes.c_uint32, ctypes.c_float, vp, vp, rbp]; lib.f3ds_region_boxes_host.restype = ctypes.c_int
        lib.f3ds_region_boxes.argtypes = [vp, ctypes.POINTER(RgbdFormat), vp, vp, ctypes.c_uint32, ctypes.c_float, ctypes.c_int, vp, vp, ctypes.c_int, rbp]
        lib.f3ds_region_boxes.restype = ctypes.c_int
    if hasattr(lib, "f3ds_region_components"):
        rkp, ckp = ctypes.POINTER(RegionComponentsResult), ctypes.POINTER(ComponentParams)
        lib.f3ds_default_component_params.argtypes = [ckp]; lib.f3ds_default_component_params.restype = None
        lib.f3ds_region_components_host.argtypes = [ctypes.POINTER(RgbdFormat), vp, vp, ctypes.c_uint32, ckp, vp, vp, sz, ctypes.POINTER(sz), rkp]
        lib.f3ds_region_components_host.restype = ctypes.c_int
        lib.f3ds_region_components_tiled.argtypes = [ctypes.POINTER(RgbdFormat), vp, vp, ctypes.c_uint32, ckp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, sz, ctypes.POINTER(sz), rkp]
        lib.f3ds_region_components_tiled.restype = ctypes.c_int
        lib.f3ds_region_components.argtypes = [vp, ctypes.POINTER(RgbdFormat), vp, vp, ctypes.c_uint32, ckp, ctypes.c_int, vp, vp, sz, ctypes.c_int, ctypes.POINTER(sz), rkp]
        lib.f3ds_region_components.restype = ctypes.c_int
    if hasattr(lib, "f3ds_region_joints"):
        rjp, jpp, fp = ctypes.POINTER(RegionJointsResult), ctypes.POINTER(JointParams), ctypes.POINTER(RgbdFormat)
        lib.f3ds_default_joint_params.argtypes = [jpp]; lib.f3ds_default_joint_params.restype = None
        lib.f3ds_region_joints_host.argtypes = [fp, vp, vp, ctypes.c_uint32, jpp, vp, sz, ctypes.POINTER(sz), vp, rjp]; lib.f3ds_region_joints_host.restype = ctypes.c_int
        lib.f3ds_region_joints.argtypes = [vp, fp, vp, vp, ctypes.c_uint32, jpp, ctypes.c_int, vp, sz, vp, ctypes.c_int, ctypes.POINTER(sz), rjp]
        lib.f3ds_region_joints.restype = ctypes.c_int
        lib.f3ds_region_joints_batch.argtypes = [ctypes.POINTER(vp), ctypes.c_int, fp, ctypes.POINTER(vp), ctypes.POINTER(vp), vp, jpp, ctypes.c_int, ctypes.POINTER(vp), vp,
                                                 ctypes.POINTER(vp), ctypes.c_int, vp, vp, vp]
        lib.f3ds_region_joints_batch.restype = ctypes.c_int
    if hasattr(lib, "f3ds_cloud_regions"):
        crp, cpp, pp = ctypes.POINTER(CloudRegionsResult), ctypes.POINTER(CloudParams), ctypes.POINTER(vp)
        lib.f3ds_default_cloud_params.argtypes = [cpp]; lib.f3ds_default_cloud_params.restype = None
        lib.f3ds_cloud_regions_host.argtypes = [vp, sz, vp, ctypes.c_uint32, cpp, vp, vp, crp]; lib.f3ds_cloud_regions_host.restype = ctypes.c_int
        lib.f3ds_cloud_regions.argtypes = [vp, vp, sz, vp, ctypes.c_uint32, cpp, ctypes.c_int, vp, vp, ctypes.c_int, crp]; lib.f3ds_cloud_regions.restype = ctypes.c_int
        lib.f3ds_cloud_regions_batch.argtypes = [pp, ctypes.c_int, pp, vp, pp, vp, cpp, ctypes.c_int, pp, pp, ctypes.c_int, vp, vp]
        lib.f3ds_cloud_regions_batch.restype = ctypes.c_int
    if hasattr(lib, "f3ds_region_table_batch"):      # the batch forms: arrays of per-frame pointers (void**), counts and results
        pp, fp, i32 = ctypes.POINTER(vp), ctypes.POINTER(RgbdFormat), ctypes.c_int
        lib.f3ds_region_table_batch.argtypes = [pp, i32, fp, pp, pp, pp, vp, i32, pp, i32, vp, vp]
        lib.f3ds_region_shapes_batch.argtypes = [pp, i32, fp, pp, pp, vp, i32, pp, i32, vp, vp]
        lib.f3ds_region_boxes_batch.argtypes = [pp, i32, fp, pp, pp, vp, ctypes.c_float, i32, pp, pp, i32, vp, vp]
        lib.f3ds_region_contacts_batch.argtypes = [pp, i32, fp, pp, pp, vp, ctypes.c_float, i32, pp, vp, i32, vp, vp, vp]
        lib.f3ds_region_components_batch.argtypes = [pp, i32, fp, pp, pp, vp, ctypes.POINTER(ComponentParams), i32, pp, pp, vp, i32, vp, vp, vp]
        for name in ("table", "shapes", "boxes", "contacts", "components"):
            getattr(lib, "f3ds_region_%s_batch" % name).restype = ctypes.c_int
    lib.f3ds_recluster.argtypes = [vp, ctypes.POINTER(Params), vp, ctypes.c_int, ctypes.POINTER(Result)]
    lib.f3ds_recluster.restype = ctypes.c_int
    lib.f3ds_evaluate.argtypes = [vp, vp, ctypes.POINTER(Performance)]; lib.f3ds_evaluate.restype = ctypes.c_int
    lib.f3ds_auto_threshold.argtypes = [vp, ctypes.POINTER(Params), vp, ctypes.c_float, ctypes.c_float, ctypes.c_float, vp, vp, sz, ctypes.POINTER(sz),
                                        ctypes.POINTER(ctypes.c_float), ctypes.POINTER(Performance), vp, ctypes.c_int, ctypes.POINTER(Result)]
    lib.f3ds_auto_threshold.restype = ctypes.c_int
    lib.f3ds_get_voxel_centroid_cloud.argtypes = [vp, vp, vp, vp, sz, ctypes.POINTER(sz)]; lib.f3ds_get_voxel_centroid_cloud.restype = ctypes.c_int
    lib.f3ds_get_supervoxels.argtypes = [vp, vp, vp, vp, vp, vp, sz, ctypes.POINTER(sz)]; lib.f3ds_get_supervoxels.restype = ctypes.c_int
    lib.f3ds_get_supervoxel_adjacency.argtypes = [vp, vp, sz, ctypes.POINTER(sz)]; lib.f3ds_get_supervoxel_adjacency.restype = ctypes.c_int
    lib.f3ds_refine_supervoxels.argtypes = [vp, ctypes.c_int]; lib.f3ds_refine_supervoxels.restype = ctypes.c_int
    lib.f3ds_get_refined_voxels.argtypes = [vp, vp, vp, sz, ctypes.POINTER(sz)]; lib.f3ds_get_refined_voxels.restype = ctypes.c_int
    lib.f3ds_get_refined_supervoxels.argtypes = [vp, vp, vp, vp, vp, vp, sz, ctypes.POINTER(sz)]; lib.f3ds_get_refined_supervoxels.restype = ctypes.c_int
    lib.f3ds_get_voxel_cloud.argtypes = [vp, vp, vp, vp, sz, ctypes.POINTER(sz)]; lib.f3ds_get_voxel_cloud.restype = ctypes.c_int
    lib.f3ds_get_debug.argtypes = [vp, ctypes.c_int, vp, sz, ctypes.POINTER(sz)]; lib.f3ds_get_debug.restype = ctypes.c_int
    lib.f3ds_get_region_adjacency.argtypes = [vp, vp, sz, ctypes.POINTER(sz)]; lib.f3ds_get_region_adjacency.restype = ctypes.c_int
    lib.f3ds_cluster_supervoxels.argtypes = [vp, ctypes.POINTER(SupervoxelSet), vp, sz, ctypes.POINTER(Params), vp, vp, ctypes.POINTER(Result)]
    lib.f3ds_cluster_supervoxels.restype = ctypes.c_int
    lib.f3ds_get_regions.argtypes = [vp, vp, vp, vp, vp, vp, sz, ctypes.POINTER(sz)]; lib.f3ds_get_regions.restype = ctypes.c_int
    if hasattr(lib, "f3ds_labels_at_thresholds"):      # (hierarchy levels; F3DS_LIB may point at an older build during A/B runs)
        lib.f3ds_labels_at_thresholds.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_int, vp]; lib.f3ds_labels_at_thresholds.restype = ctypes.c_int
        lib.f3ds_labels_at_thresholds_batch.argtypes = [ctypes.POINTER(vp), ctypes.c_int, vp, ctypes.c_int, ctypes.POINTER(vp), ctypes.c_int, vp]
        lib.f3ds_labels_at_thresholds_batch.restype = ctypes.c_int
    if hasattr(lib, "f3ds_evaluate_levels"):      # (scores of hierarchy levels)
        lib.f3ds_evaluate_levels.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_int, vp, vp]; lib.f3ds_evaluate_levels.restype = ctypes.c_int
        lib.f3ds_evaluate_levels_batch.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.POINTER(vp), ctypes.c_int, vp, ctypes.c_int, vp, vp]
        lib.f3ds_evaluate_levels_batch.restype = ctypes.c_int
        lib.f3ds_best_level.argtypes = [vp, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]; lib.f3ds_best_level.restype = ctypes.c_int
        lib.f3ds_get_merge_tree.argtypes = [vp, vp, vp, vp, sz, ctypes.POINTER(sz)]; lib.f3ds_get_merge_tree.restype = ctypes.c_int
    lib.f3ds_get_region_voxels.argtypes = [vp, vp, vp, vp, sz, ctypes.POINTER(sz)]; lib.f3ds_get_region_voxels.restype = ctypes.c_int
    lib.f3ds_multi_create.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]; lib.f3ds_multi_create.restype = ctypes.c_int
    lib.f3ds_multi_destroy.argtypes = [vp]; lib.f3ds_multi_destroy.restype = None
    lib.f3ds_multi_devices.argtypes = [vp]; lib.f3ds_multi_devices.restype = ctypes.c_int
    lib.f3ds_multi_device_of_frame.argtypes = [vp, ctypes.c_int]; lib.f3ds_multi_device_of_frame.restype = ctypes.c_int
    lib.f3ds_multi_segment.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.c_int, ctypes.POINTER(Params), ctypes.POINTER(vp), ctypes.POINTER(Result)]
    lib.f3ds_multi_segment.restype = ctypes.c_int
    lib.f3ds_multi_submit.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.c_int, ctypes.POINTER(Params), ctypes.POINTER(vp), ctypes.POINTER(Result), ctypes.POINTER(ctypes.c_int)]
    lib.f3ds_multi_submit.restype = ctypes.c_int
    lib.f3ds_multi_collect.argtypes = [vp, ctypes.c_int]; lib.f3ds_multi_collect.restype = ctypes.c_int
    lib.f3ds_multi_reserve.argtypes = [vp, sz]; lib.f3ds_multi_reserve.restype = ctypes.c_int
    lib.f3ds_multi_gathered_labels.argtypes = [vp]; lib.f3ds_multi_gathered_labels.restype = vp
    if hasattr(lib, "f3ds_multi_gathered_labels_of"):
        lib.f3ds_multi_gathered_labels_of.argtypes = [vp, ctypes.c_int]; lib.f3ds_multi_gathered_labels_of.restype = vp
    lib.f3ds_multi_last_error.restype = ctypes.c_char_p
    lib.f3ds_stream_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]; lib.f3ds_stream_create.restype = ctypes.c_int
    lib.f3ds_stream_destroy.argtypes = [vp]; lib.f3ds_stream_destroy.restype = None
    lib.f3ds_stream_buffer.argtypes = [vp, sz, ctypes.POINTER(vp)]; lib.f3ds_stream_buffer.restype = ctypes.c_int
    lib.f3ds_stream_submit.argtypes = [vp, vp, sz, ctypes.POINTER(Params), ctypes.c_uint64]; lib.f3ds_stream_submit.restype = ctypes.c_int
    lib.f3ds_stream_next.argtypes = [vp, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(Result), ctypes.c_int]
    lib.f3ds_stream_next.restype = ctypes.c_int
    lib.f3ds_stream_peek.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(Result), ctypes.c_int]
    lib.f3ds_stream_peek.restype = ctypes.c_int
    lib.f3ds_stream_pending.argtypes = [vp]; lib.f3ds_stream_pending.restype = ctypes.c_int
    lib.f3ds_pcd_read.argtypes = [ctypes.c_char_p, vp, vp, sz, ctypes.POINTER(sz), u32p, u32p]; lib.f3ds_pcd_read.restype = ctypes.c_int
    lib.f3ds_pcd_write.argtypes = [ctypes.c_char_p, vp, vp, vp, sz, ctypes.c_int]; lib.f3ds_pcd_write.restype = ctypes.c_int
    lib.f3ds_synth_frame.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp]
    lib.f3ds_synth_frame.restype = ctypes.c_int
    lib.f3ds_label_color.argtypes = [ctypes.c_uint32]; lib.f3ds_label_color.restype = ctypes.c_uint32
    if path is None:
        _lib = lib
    return lib


def source_stamp():
    """First 16 hex digits of the SHA-256 over the library's sources as csrc/Makefile hashes them (every *.hip *.inc *.h *.cpp of
    csrc/ but the generated stamp header, in byte-wise name order, then include/f3ds.h and include/f3ds_clustering.hpp)."""
    import glob
    import hashlib
    csrc = os.path.join(_HERE, "csrc")
    names = sorted(os.path.basename(f) for pat in ("*.hip", "*.inc", "*.h", "*.cpp") for f in glob.glob(os.path.join(csrc, pat)))
    files = [os.path.join(csrc, n) for n in names if n != "f3ds_build_stamp.h"]
    inc = os.path.join(os.path.dirname(_HERE), "include")
    files += [os.path.join(inc, "f3ds.h"), os.path.join(inc, "f3ds_clustering.hpp")]
    h = hashlib.sha256()
    for f in files:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def library_stamp(lib=None):
    """The stamp the loaded libf3ds.so was built from (f3ds_version_string: 'f3ds 1.2.0 src:<stamp>[ +whatif]')."""
    text = (lib or load_library()).f3ds_version_string().decode()
    return text.split("src:")[1].split()[0], text


def merge_layout_info(n_edges, waves=8, keys_in_lds=2):
    """f3ds_merge_layout_info: (dynamic LDS bytes, rows a speculative second merge may absorb, edge slots, fits?) of d_merge_il_t<waves, keys_in_lds>
    for a frame with n_edges adjacencies.  Host arithmetic only."""
    out = (ctypes.c_uint32 * 4)()
    lib = load_library()
    _check(lib, lib.f3ds_merge_layout_info(ctypes.c_uint32(int(n_edges)), int(waves), int(keys_in_lds), out))
    return int(out[0]), int(out[1]), int(out[2]), bool(out[3])


def constant(name):
    """f3ds_constant: a limit of the kernels or of the host's batch-wide decisions by name ("NT_RING1", "EDGE_MULT", "d_reseed::BLOCK", ...), from the constant
    the code itself uses.  Host arithmetic only.  The seed kernels' floating margins come back as floats."""
    out = ctypes.c_uint64()
    lib = load_library()
    _check(lib, lib.f3ds_constant(str(name).encode(), ctypes.byref(out)))
    if name in ("SEED_NN_MARGIN", "SEED_NN_ULP", "SEED_PRUNE_MARGIN"):
        return struct.unpack("<d", struct.pack("<Q", out.value))[0]
    return int(out.value)


def constants():
    """Every name f3ds_constant knows, with its value."""
    lib = load_library()
    lib.f3ds_constant_name.restype = ctypes.c_char_p
    names, i = [], 0
    while True:
        n = lib.f3ds_constant_name(ctypes.c_size_t(i))
        if n is None:
            return {k: constant(k) for k in names}
        names.append(n.decode()); i += 1


def stage0_plan(max_depth, max_points, n_contexts, vox_tiles=1, sort_pairs=0):
    """f3ds_stage0_plan: (tile path?, tile bits, index bits of a one-word sort key or -1 for (key, index) pairs, sort key bits without the index) of a batch
    call with fresh contexts.  vox_tiles: F3DS_VOX_TILES (1: unset).  Host arithmetic only."""
    out = (ctypes.c_int32 * 4)()
    lib = load_library()
    _check(lib, lib.f3ds_stage0_plan(int(max_depth), ctypes.c_uint32(int(max_points)), int(n_contexts), int(vox_tiles), int(sort_pairs), out))
    return bool(out[0]), int(out[1]), int(out[2]), int(out[3])


CAP_EDGES, CAP_EVENTS, CAP_LEAF_POOL, CAP_ILIST = 0, 1, 2, 3


def policy_capacity(what, count, mult, n_seeds=0, slack=32):
    """f3ds_policy_capacity: entries of the adjacency list (CAP_EDGES: count seeds), the weight history (CAP_EVENTS: count edges), the leaf pool (CAP_LEAF_POOL:
    count seeds) or the incident-list pool (CAP_ILIST: count edges, n_seeds, F3DS_ILIST_SLACK = slack) at the multiplier `mult`."""
    out = ctypes.c_uint32()
    lib = load_library()
    _check(lib, lib.f3ds_policy_capacity(int(what), ctypes.c_uint32(int(count)), ctypes.c_uint32(int(n_seeds)), ctypes.c_uint32(int(mult)), ctypes.c_uint32(int(slack)), ctypes.byref(out)))
    return int(out.value)


def policy_grow(mult, cap):
    """f3ds_policy_grow: a buffer's multiplier after an overflow (unchanged once it has reached `cap`)."""
    out = ctypes.c_uint32()
    lib = load_library()
    _check(lib, lib.f3ds_policy_grow(ctypes.c_uint32(int(mult)), ctypes.c_uint32(int(cap)), ctypes.byref(out)))
    return int(out.value)


def policy_dense_penalty(penalty):
    """f3ds_policy_dense_penalty: the calls a context stays off the tile path after its next refusal."""
    lib = load_library()
    lib.f3ds_policy_dense_penalty.restype = ctypes.c_uint32
    return int(lib.f3ds_policy_dense_penalty(ctypes.c_uint32(int(penalty))))


def policy_launch(frames, normals_forced=0, grid_target=None, grid_cap_forced=0):
    """f3ds_policy_launch: (threads of the normals kernel, workgroups per frame of a streaming kernel, of a gathering kernel) in a call of `frames` frames."""
    out = (ctypes.c_uint32 * 3)()
    lib = load_library()
    target = constant("GRID_TARGET") if grid_target is None else grid_target
    _check(lib, lib.f3ds_policy_launch(int(frames), int(normals_forced), ctypes.c_uint32(int(target)), ctypes.c_uint32(int(grid_cap_forced)), out))
    return int(out[0]), int(out[1]), int(out[2])


def policy_stage_layout(fixed_bytes, stage_rows, row_bytes, first_rows):
    """f3ds_policy_stage_layout: ([[at, rows_at, first] per frame], first_bytes, total) of a label-image batch call's staging.  stage_rows: None for a call without rows."""
    n = len(fixed_bytes)
    arr = ctypes.c_size_t * n
    slots = (ctypes.c_size_t * (3 * n))(); first, total = ctypes.c_size_t(), ctypes.c_size_t()
    lib = load_library()
    _check(lib, lib.f3ds_policy_stage_layout(ctypes.c_size_t(n), arr(*fixed_bytes), None if stage_rows is None else arr(*stage_rows), ctypes.c_size_t(int(row_bytes)),
                                             ctypes.c_size_t(int(first_rows)), slots, ctypes.byref(first), ctypes.byref(total)))
    return [[int(slots[3 * i]), int(slots[3 * i + 1]), int(slots[3 * i + 2])] for i in range(n)], int(first.value), int(total.value)


def check_library_is_current(lib=None):
    """Raise if the loaded libf3ds.so was not built from the sources beside it (a stale prebuilt .so travels to the GPU box with the
    snapshot; measuring or testing it would describe some other code).  Skipped when F3DS_LIB points at another build on purpose."""
    if _dev_env("F3DS_LIB"):
        return
    have, text = library_stamp(lib)
    want = source_stamp()
    if have != want:
        raise ImportError("libf3ds.so is stale: built from sources %s, the tree holds %s (%s) -- rebuild with make -C %s" % (have, want, text, os.path.join(_HERE, "csrc")))


(OK, ERR_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_DEPTH, ERR_LOGIC, ERR_RANGE, ERR_UNSUPPORTED, ERR_IO, ERR_EQ_BIN,
 ERR_CAPACITY, ERR_BUSY, ERR_EMPTY, ERR_OUT_OF_RANGE) = (0, -1, -2, -3, -4, -5, -6, -7, -8, -9, -10, -11, -12, -13)       # include/f3ds.h:37-56


def _check(lib, rc):
    if rc == 0:
        return
    text = lib.f3ds_strerror(rc).decode()
    if rc == -3:
        text += " [" + lib.f3ds_last_hip_error().decode() + "]"
    if rc == -5:
        raise LogicError(rc, text)
    if rc == -6:
        raise ValueError(text)
    if rc == -13:
        raise IndexError(text)      # std::out_of_range of the reference (map::at, all_thresh bounds)
    raise F3dsError(rc, text)


def _two_call(lib, fn, lead, outs, tail=()):
    """The two-call protocol of the C getters, ``fn(*lead, outputs..., cap, *tail, &n)``: once with null outputs for the count n, then with one fresh
    array per ``(dtype, trailing shape)`` of ``outs``, n entries each.  Returns the list of arrays."""
    n = ctypes.c_size_t()
    _check(lib, fn(*lead, *[None] * len(outs), 0, *tail, ctypes.byref(n)))
    arrays = [np.zeros((n.value,) + tuple(shape), dtype) for dtype, shape in outs]
    _check(lib, fn(*lead, *[a.ctypes.data for a in arrays], n.value, *tail, ctypes.byref(n)))
    return arrays


_U32, _F32, _XYZ, _PAIR = (np.uint32, ()), (np.float32, ()), (np.float32, (3,)), (np.uint32, (2,))      # output kinds of _two_call


def _label_buffer(buf, n, what, name="labels_out"):
    """The host array a call writes one uint32 per ``what`` into: a fresh one, or the caller's own after a check."""
    if buf is None:
        return np.empty(n, np.uint32)
    if not (isinstance(buf, np.ndarray) and buf.dtype == np.uint32 and buf.flags.c_contiguous and buf.size == n):
        raise ValueError("%s must be a contiguous uint32 array with one entry per %s" % (name, what))
    return buf


class _Handle:
    """close() / __del__ of an object that owns a C handle; ``_destroy`` names the library function that releases it."""
    _destroy = None

    def close(self):
        if getattr(self, "handle", None):
            getattr(self.lib, self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_supervoxels(segm):
    """{label: dict(voxels_xyz (n,3) f32, voxels_rgba (n,) u32, centroid (3,), normal (3,))} -- the shape of the reference's
    ``std::map<uint32_t, pcl::Supervoxel::Ptr>`` -- -> dict of the arrays f3ds_supervoxel_set points at (rows in the dict's own order)."""
    labels = np.array(list(segm.keys()), np.uint32)
    counts = [len(np.asarray(segm[k]["voxels_xyz"]).reshape(-1, 3)) for k in segm]
    off = np.zeros(len(labels) + 1, np.uint32)
    off[1:] = np.cumsum(counts)
    xyz = np.concatenate([np.asarray(segm[k]["voxels_xyz"], np.float32).reshape(-1, 3) for k in segm]) if len(labels) else np.zeros((0, 3), np.float32)
    rgba = np.concatenate([np.asarray(segm[k]["voxels_rgba"], np.uint32).reshape(-1) for k in segm]) if len(labels) else np.zeros(0, np.uint32)
    cent = np.array([np.asarray(segm[k]["centroid"], np.float32)[:3] for k in segm], np.float32).reshape(-1, 3)
    nrm = np.array([np.asarray(segm[k]["normal"], np.float32)[:3] for k in segm], np.float32).reshape(-1, 3)
    return dict(label=labels, voxel_offset=off, voxel_xyz=np.ascontiguousarray(xyz), voxel_rgba=np.ascontiguousarray(rgba), centroid_xyz=cent, normal=nrm)


def default_params(**kw):
    lib = load_library()
    p = Params()
    lib.f3ds_default_params(ctypes.byref(p))
    for k, v in kw.items():
        if k == "lambda":
            k = "lambda_"
        if not hasattr(p, k):
            raise TypeError("unknown parameter %r" % k)
        setattr(p, k, v)
    return p


def launch_params(**kw):
    """The reference's canonical flags ``--CVX --AL -t 0.2`` (launch/supervoxel_clustering.launch:3-6)."""
    d = dict(geom_metric=CONVEX_NORMALS_DIFF, merging=ADAPTIVE_LAMBDA, threshold=0.2)
    d.update(kw)
    return default_params(**d)


def device_count():
    return load_library().f3ds_device_count()


# ---- host helpers either side of the path -------------------------------------------------------
def read_pcd(path, with_labels=False):
    """PCD v0.7 (ascii / binary / binary_compressed) -> (N,4) float32 view of {x,y,z,rgba-bits}."""
    lib = load_library()
    n = ctypes.c_size_t(); w = ctypes.c_uint32(); h = ctypes.c_uint32()
    _check(lib, lib.f3ds_pcd_read(path.encode(), None, None, 0, ctypes.byref(n), ctypes.byref(w), ctypes.byref(h)))
    pts = np.zeros((n.value, 4), np.float32)
    labels = np.zeros(n.value, np.uint32) if with_labels else None
    _check(lib, lib.f3ds_pcd_read(path.encode(), pts.ctypes.data, labels.ctypes.data if with_labels else None, n.value,
                                  ctypes.byref(n), None, None))
    return (pts, labels) if with_labels else pts


def write_pcd(path, xyz, rgba=None, labels=None, binary=True):
    lib = load_library()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    rgba = None if rgba is None else np.ascontiguousarray(rgba, np.uint32)
    labels = None if labels is None else np.ascontiguousarray(labels, np.uint32)
    _check(lib, lib.f3ds_pcd_write(path.encode(), xyz.ctypes.data, None if rgba is None else rgba.ctypes.data,
                                   None if labels is None else labels.ctypes.data, n, 1 if binary else 0))


def synth_frame(kind, seed, width, height, nan_permille=0):
    """Deterministic synthetic frame; (N,4) float32, column 3 = rgba bits."""
    lib = load_library()
    pts = np.zeros((width * height, 4), np.float32)
    _check(lib, lib.f3ds_synth_frame(kind, seed, width, height, nan_permille, pts.ctypes.data))
    return pts


def label_color(label):
    return load_library().f3ds_label_color(label)


# ---- RGB-D frames ---------------------------------------------------------------------------------
_DEPTH_DTYPE = {DEPTH_U16: np.uint16, DEPTH_F32: np.float32}


def _rgbd_images(fmt, depth, color):
    """(format with the pitches of these arrays, depth array, colour array): the images as the library reads them.  Rows may be strided (a
    view of a wider image): the row stride becomes the pitch; an array whose pixels are not contiguous within a row is copied."""
    w, h = int(fmt.width), int(fmt.height)
    if fmt.depth_type not in _DEPTH_DTYPE or fmt.color_format not in (COLOR_RGB8, COLOR_RGBA8, COLOR_PACKED):
        raise F3dsError(ERR_ARG, "unknown depth type or colour format")
    d = np.asarray(depth, _DEPTH_DTYPE[fmt.depth_type])
    if fmt.color_format == COLOR_PACKED:
        c = np.asarray(color, np.uint32)
        cshape, cinner = (h, w), (c.itemsize,)
    else:
        ch = 3 if fmt.color_format == COLOR_RGB8 else 4
        c = np.asarray(color, np.uint8)
        cshape, cinner = (h, w, ch), (ch, 1)
    if d.shape != (h, w) or c.shape != cshape:
        raise ValueError("depth must be (height, width) and colour %r, got %r and %r" % (cshape, d.shape, c.shape))
    if h > 1 and w > 0 and (d.strides[1] != d.itemsize or d.strides[0] < w * d.itemsize):
        d = np.ascontiguousarray(d)
    if h > 1 and w > 0 and (tuple(c.strides[1:]) != cinner or c.strides[0] < w * cinner[0]):
        c = np.ascontiguousarray(c)
    if h <= 1 or w == 0:
        d, c = np.ascontiguousarray(d), np.ascontiguousarray(c)
    f = fmt.copy()
    f.depth_pitch = 0 if d.flags.c_contiguous else d.strides[0]
    f.color_pitch = 0 if c.flags.c_contiguous else c.strides[0]
    return f, d, c


def deproject(fmt, depth, color):
    """f3ds_deproject: the (N, 4) float32 records (x, y, z, rgba bits; N = width * height, pixel (u, v) at row v * width + u) that
    Context.segment_rgbd builds on the device, bit for bit.  Host arithmetic only."""
    lib = load_library()
    f, d, c = _rgbd_images(fmt, depth, color)
    pts = np.empty((int(fmt.width) * int(fmt.height), 4), np.float32)
    _check(lib, lib.f3ds_deproject(ctypes.byref(f), d.ctypes.data, c.ctypes.data, pts.ctypes.data))
    return pts


# ---- label tracker -----------------------------------------------------------------------------------
def default_track_params(**kw):
    p = TrackParams()
    load_library().f3ds_default_track_params(ctypes.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError("unknown parameter %r" % k)
        setattr(p, k, v)
    return p


def _pose12(pose):
    """None, or the 12 floats of a row-major 3 x 4 pose (a 4 x 4 matrix gives its first three rows)"""
    if pose is None:
        return None
    m = np.asarray(pose, np.float32)
    if m.shape == (4, 4):
        m = m[:3]
    if m.size != 12:
        raise ValueError("a pose is 12 floats (row-major 3 x 4) or a 4 x 4 matrix")
    return np.ascontiguousarray(m, np.float32).reshape(12)


def track_reproject(fmt, points, pose=None):
    """f3ds_track_reproject: (pixel index in the previous frame or -1 (int32), depth there (float32)) of every (N, 4) float32 record under `pose`
    (p_prev = R p_cur + t; None = identity).  Host arithmetic only: what Tracker.update does per labelled pixel on the device."""
    lib = load_library()
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    m = _pose12(pose)
    pixel, zp = np.empty(len(pts), np.int32), np.empty(len(pts), np.float32)
    _check(lib, lib.f3ds_track_reproject(ctypes.byref(fmt), None if m is None else m.ctypes.data, pts.ctypes.data, len(pts), pixel.ctypes.data, zp.ctypes.data))
    return pixel, zp


def track_assign(size, entries, prev_id, next_id, params=None):
    """f3ds_track_assign: (id of every region (uint32, NO_LABEL for an empty one), next_id afterwards, TrackResult) from the regions' sizes, the vote
    entries ((n, 3) uint32 rows: region, previous slot, votes) and the previous slots' ids.  Host arithmetic only."""
    lib = load_library()
    size = np.ascontiguousarray(size, np.uint32).reshape(-1)
    entries = np.ascontiguousarray(entries, np.uint32).reshape(-1, 3)
    prev_id = np.ascontiguousarray(prev_id, np.uint32).reshape(-1)
    ids = np.full(len(size), NO_LABEL, np.uint32)
    nxt, res = ctypes.c_uint32(int(next_id)), TrackResult()
    _check(lib, lib.f3ds_track_assign(ctypes.byref(params) if params is not None else None, size.ctypes.data, len(size), entries.ctypes.data, len(entries),
                                      prev_id.ctypes.data, len(prev_id), ctypes.byref(nxt), ids.ctypes.data, ctypes.byref(res)))
    return ids, int(nxt.value), res


class Tracker(_Handle):
    """f3ds_tracker (include/f3ds.h): persistent ids for the regions of consecutive RGB-D frames.  Not thread-safe; one per camera."""

    _destroy = "f3ds_tracker_destroy"

    def __init__(self, device=0, params=None):
        self.lib = load_library()
        h = ctypes.c_void_p()
        _check(self.lib, self.lib.f3ds_tracker_create(device, ctypes.byref(params) if params is not None else None, ctypes.byref(h)))
        self.handle = h
        self.device = device
        self.result = TrackResult()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_stream(self, hip_stream_ptr):
        _check(self.lib, self.lib.f3ds_tracker_set_stream(self.handle, ctypes.c_void_p(hip_stream_ptr)))

    def reset(self):
        """Forget the previous frame (the next update matches nothing); ids given out so far are not given out again."""
        _check(self.lib, self.lib.f3ds_tracker_reset(self.handle))

    def update(self, depth, labels, n_regions, fmt, pose=None, ids_out=None, on_device=False):
        """f3ds_tracker_update: the track id of every pixel.  depth: (height, width) uint16 / float32 as ``fmt`` says (rows may be strided), labels: one
        uint32 per pixel as segment_rgbd wrote them, n_regions: ``Context.result.n_regions`` of that call; or device pointers (ints, the depth pitch
        of ``fmt`` applies) with ``on_device=True``, ``ids_out`` then a device pointer too.  pose: 12 floats (row-major 3 x 4) or a 4 x 4 matrix that
        takes this frame's camera coordinates to the previous frame's; None = the camera has not moved.  ``self.result`` holds the counts."""
        n = int(fmt.width) * int(fmt.height)
        m = _pose12(pose)
        mp = None if m is None else m.ctypes.data
        if on_device:
            _check(self.lib, self.lib.f3ds_tracker_update(self.handle, ctypes.byref(fmt), ctypes.c_void_p(int(depth)), ctypes.c_void_p(int(labels)), int(n_regions), 1, mp,
                                                          ctypes.c_void_p(int(ids_out)), 1, ctypes.byref(self.result)))
            return None
        if fmt.depth_type not in _DEPTH_DTYPE:
            raise F3dsError(ERR_ARG, "unknown depth type")
        d = np.asarray(depth, _DEPTH_DTYPE[fmt.depth_type])
        if d.shape != (int(fmt.height), int(fmt.width)):
            raise ValueError("depth must be (height, width), got %r" % (d.shape,))
        if d.shape[0] <= 1 or d.strides[1] != d.itemsize or d.strides[0] < d.shape[1] * d.itemsize:
            d = np.ascontiguousarray(d)
        f = fmt.copy()
        f.depth_pitch = 0 if d.flags.c_contiguous else d.strides[0]
        lab = np.ascontiguousarray(labels, np.uint32).reshape(-1)
        if lab.size != n:
            raise ValueError("labels must hold one entry per pixel")
        ids = _label_buffer(ids_out, n, "pixel", "ids_out")
        _check(self.lib, self.lib.f3ds_tracker_update(self.handle, ctypes.byref(f), d.ctypes.data, lab.ctypes.data, int(n_regions), 0, mp, ids.ctypes.data, 0,
                                                      ctypes.byref(self.result)))
        return ids

    def ids(self):
        """f3ds_tracker_get_ids: the track id of every region of the last update (NO_LABEL for a region without a labelled pixel); LogicError before any."""
        return _two_call(self.lib, self.lib.f3ds_tracker_get_ids, [self.handle], [_U32])[0]


# ---- region table --------------------------------------------------------------------------------------
def _region_inputs(fmt, depth, labels, color):
    """(format with the pitches of these arrays, depth array, colour array or None, labels) of the host forms of the region table"""
    n = int(fmt.width) * int(fmt.height)
    if color is not None:
        f, d, c = _rgbd_images(fmt, depth, color)
    else:
        if fmt.depth_type not in _DEPTH_DTYPE:
            raise F3dsError(ERR_ARG, "unknown depth type")
        d = np.asarray(depth, _DEPTH_DTYPE[fmt.depth_type])
        if d.shape != (int(fmt.height), int(fmt.width)):
            raise ValueError("depth must be (height, width), got %r" % (d.shape,))
        if d.shape[0] <= 1 or d.strides[1] != d.itemsize or d.strides[0] < d.shape[1] * d.itemsize:
            d = np.ascontiguousarray(d)
        f, c = fmt.copy(), None
        f.depth_pitch = 0 if d.flags.c_contiguous else d.strides[0]
    lab = np.ascontiguousarray(labels, np.uint32).reshape(-1)
    if lab.size != n:
        raise ValueError("labels must hold one entry per pixel")
    return f, d, c, lab


def _region_rows(buf, n_regions):
    if buf is None:
        return np.empty(int(n_regions), REGION_ROW_DTYPE)
    if not (isinstance(buf, np.ndarray) and buf.dtype == REGION_ROW_DTYPE and buf.flags.c_contiguous and buf.size == int(n_regions)):
        raise ValueError("rows_out must be a contiguous REGION_ROW_DTYPE array with one entry per region")
    return buf


def region_table_host(depth, labels, n_regions, fmt, color=None):
    """f3ds_region_table_host: (rows, RegionTableResult) -- one REGION_ROW_DTYPE row per region of the label image: pixel count, first pixel, pixel box, box of
    the points, centroid and mean colour (0 without ``color``).  Host arithmetic only: what Context.region_table computes on the device, bit for bit."""
    lib = load_library()
    f, d, c, lab = _region_inputs(fmt, depth, labels, color)
    rows, res = _region_rows(None, n_regions), RegionTableResult()
    _check(lib, lib.f3ds_region_table_host(ctypes.byref(f), d.ctypes.data, None if c is None else c.ctypes.data, lab.ctypes.data, int(n_regions),
                                           rows.ctypes.data if len(rows) else None, ctypes.byref(res)))
    return rows, res


# ---- region contacts -------------------------------------------------------------------------------
_CONTACT_ROWS_FIRST = 1024      # rows the first call of the package's two functions has room for; more: the buffer grows from n_out and the call is repeated


def _contact_rows(call, rows_out, dtype=REGION_CONTACT_DTYPE):
    """the rows of call(pointer, cap, byref(n_out)) -> rc: into ``rows_out`` (too small: CapacityError), or into a buffer grown from n_out"""
    n_out = ctypes.c_size_t(0)
    if rows_out is not None:
        if not (isinstance(rows_out, np.ndarray) and rows_out.dtype == dtype and rows_out.flags.c_contiguous and rows_out.ndim == 1):
            raise ValueError("rows_out must be a contiguous one-dimensional array of the rows' dtype (%d bytes per row)" % dtype.itemsize)
        rc = call(rows_out.ctypes.data if len(rows_out) else None, len(rows_out), ctypes.byref(n_out))
        if rc == 0 and n_out.value > len(rows_out):      # (an empty buffer is a NULL pointer: the call only counted)
            rc = ERR_CAPACITY
        return rc, rows_out[:n_out.value] if rc == 0 else None
    rows = np.empty(_CONTACT_ROWS_FIRST, dtype)
    rc = call(rows.ctypes.data, len(rows), ctypes.byref(n_out))
    if rc == ERR_CAPACITY:
        rows = np.empty(n_out.value, dtype)
        rc = call(rows.ctypes.data, len(rows), ctypes.byref(n_out))
    return rc, rows[:n_out.value].copy() if rc == 0 else None


def region_contacts_host(depth, labels, n_regions, fmt, depth_tol=0.05):
    """f3ds_region_contacts_host: (rows, RegionContactsResult) -- one REGION_CONTACT_DTYPE row per pair of regions (a < b) of the label image that touch
    (4-connectivity), by a and then b: contact pairs, how many of them are close in depth (|za - zb| <= depth_tol * min(za, zb)), in how many of the others a
    is in front, how many are horizontal, the first pixel and the mean gap.  Host arithmetic only: what Context.region_contacts computes on the device, bit
    for bit."""
    lib = load_library()
    f, d, _, lab = _region_inputs(fmt, depth, labels, None)
    res = RegionContactsResult()
    rc, rows = _contact_rows(lambda ptr, cap, n_out: lib.f3ds_region_contacts_host(ctypes.byref(f), d.ctypes.data, lab.ctypes.data, int(n_regions), float(depth_tol), ptr, cap,
                                                                                    n_out, ctypes.byref(res)), None)
    _check(lib, rc)
    return rows, res


# ---- region shapes ---------------------------------------------------------------------------------
def _shape_rows(buf, n_regions):
    if buf is None:
        return np.empty(int(n_regions), REGION_SHAPE_DTYPE)
    if not (isinstance(buf, np.ndarray) and buf.dtype == REGION_SHAPE_DTYPE and buf.flags.c_contiguous and buf.size == int(n_regions)):
        raise ValueError("rows_out must be a contiguous REGION_SHAPE_DTYPE array with one entry per region")
    return buf


def region_shapes_host(depth, labels, n_regions, fmt):
    """f3ds_region_shapes_host: (rows, RegionShapesResult) -- one REGION_SHAPE_DTYPE row per region of the label image: pixel count, centroid, covariance of
    the points, its eigenvalues (ascending), the normal and plane_d of the plane through the centroid, the long axis and the surface variation.  Host
    arithmetic only: what Context.region_shapes computes on the device, bit for bit."""
    lib = load_library()
    f, d, _, lab = _region_inputs(fmt, depth, labels, None)
    rows, res = _shape_rows(None, n_regions), RegionShapesResult()
    _check(lib, lib.f3ds_region_shapes_host(ctypes.byref(f), d.ctypes.data, lab.ctypes.data, int(n_regions), rows.ctypes.data if len(rows) else None, ctypes.byref(res)))
    return rows, res


# ---- region boxes ----------------------------------------------------------------------------------
def _box_rows(buf, n_regions):
    if buf is None:
        return np.empty(int(n_regions), REGION_BOX_DTYPE)
    if not (isinstance(buf, np.ndarray) and buf.dtype == REGION_BOX_DTYPE and buf.flags.c_contiguous and buf.size == int(n_regions)):
        raise ValueError("rows_out must be a contiguous REGION_BOX_DTYPE array with one entry per region")
    return buf


def region_boxes_host(depth, labels, n_regions, fmt, plane_tol=0.01, want_shapes=False):
    """f3ds_region_boxes_host: (rows, RegionBoxesResult), or (rows, shapes, RegionBoxesResult) with ``want_shapes`` -- one REGION_BOX_DTYPE row per region
    of the label image: the box of the region's points along the region's own axes (the normal, the long axis of its shape row and their cross product),
    the count of pixels within ``plane_tol`` metres of the region's plane and the mean distance to it; shapes: the REGION_SHAPE_DTYPE rows of
    region_shapes_host, the same bits.  Host arithmetic only: what Context.region_boxes computes on the device, bit for bit."""
    lib = load_library()
    f, d, _, lab = _region_inputs(fmt, depth, labels, None)
    rows, res = _box_rows(None, n_regions), RegionBoxesResult()
    shapes = _shape_rows(None, n_regions) if want_shapes else None
    _check(lib, lib.f3ds_region_boxes_host(ctypes.byref(f), d.ctypes.data, lab.ctypes.data, int(n_regions), float(plane_tol), rows.ctypes.data if len(rows) else None,
                                           shapes.ctypes.data if want_shapes and len(shapes) else None, ctypes.byref(res)))
    return (rows, shapes, res) if want_shapes else (rows, res)


# ---- region rows of a point cloud --------------------------------------------------------------------
def default_cloud_params(**overrides):
    p = CloudParams()
    load_library().f3ds_default_cloud_params(ctypes.byref(p))
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


def _cloud_rows(buf, n_regions):
    if buf is None:
        return np.empty(int(n_regions), CLOUD_REGION_DTYPE)
    if not (isinstance(buf, np.ndarray) and buf.dtype == CLOUD_REGION_DTYPE and buf.flags.c_contiguous and buf.size == int(n_regions)):
        raise ValueError("rows_out must be a contiguous CLOUD_REGION_DTYPE array with one entry per region")
    return buf


def _cloud_inputs(points, labels):
    """(records as (n, 4) f32 or None, labels as (n,) u32) of a host caller; points: (n, 4) float32 records (the colour word's bits in column 3), or None"""
    lab = np.ascontiguousarray(labels, np.uint32).reshape(-1)
    if points is None:
        return None, lab
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    if len(pts) != len(lab):
        raise ValueError("one label per point is required")
    return pts, lab


def _ptr(a):
    return None if a is None or not a.size else a.ctypes.data


def cloud_regions_host(points, labels, n_regions, params=None, want_boxes=False):
    """f3ds_cloud_regions_host: (rows, CloudRegionsResult), or (rows, boxes, CloudRegionsResult) with ``want_boxes`` -- one CLOUD_REGION_DTYPE row per region
    of a labelled cloud: points (n, 4) float32 records as Context.segment takes them, labels n uint32 (< n_regions or NO_LABEL); boxes: REGION_BOX_DTYPE rows
    by the definition of region_boxes_host with the cloud rows' shape fields.  params: CloudParams (None: the defaults).  Host arithmetic only: what
    Context.cloud_regions computes on the device, bit for bit."""
    lib = load_library()
    pts, lab = _cloud_inputs(points, labels)
    rows, res = _cloud_rows(None, n_regions), CloudRegionsResult()
    boxes = _box_rows(None, n_regions) if want_boxes else None
    keep = np.zeros(4, np.float32)      # (an empty cloud still has an address)
    _check(lib, lib.f3ds_cloud_regions_host(_ptr(pts) or keep.ctypes.data, len(lab), _ptr(lab) or keep.ctypes.data, int(n_regions), ctypes.byref(params) if params is not None else None,
                                            _ptr(rows), _ptr(boxes) if want_boxes else None, ctypes.byref(res)))
    return (rows, boxes, res) if want_boxes else (rows, res)


# ---- region joints ---------------------------------------------------------------------------------
def default_joint_params(**overrides):
    p = JointParams()
    load_library().f3ds_default_joint_params(ctypes.byref(p))
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


def region_joints_host(depth, labels, n_regions, fmt, params=None, want_shapes=False, rows_out=None):
    """f3ds_region_joints_host: (rows, RegionJointsResult), or (rows, shapes, RegionJointsResult) with ``want_shapes`` -- one REGION_JOINT_DTYPE row per pair of
    regions (a < b) of the label image that touch, by a and then b: the contacts' n_pairs and n_close, centroid, direction and spread of the border's samples
    (both points of every close pair), the cosine between the two regions' planes, the reference's delta_g, the distances of each centroid from the other
    region's plane and of the border centroid from both, and ``kind`` (JOINT_OCCLUSION / _COPLANAR / _CONVEX / _CONCAVE, | JOINT_REF_CONVEX).  ``params``: a
    JointParams (None: the defaults); shapes: the REGION_SHAPE_DTYPE rows of region_shapes_host, the same bits.  Host arithmetic only: what
    Context.region_joints computes on the device, bit for bit."""
    lib = load_library()
    f, d, _, lab = _region_inputs(fmt, depth, labels, None)
    res = RegionJointsResult()
    shapes = _shape_rows(None, n_regions) if want_shapes else None
    sp = shapes.ctypes.data if want_shapes and len(shapes) else None
    pp = ctypes.byref(params) if params is not None else None
    rc, rows = _contact_rows(lambda ptr, cap, n_out: lib.f3ds_region_joints_host(ctypes.byref(f), d.ctypes.data, lab.ctypes.data, int(n_regions), pp, ptr, cap, n_out, sp,
                                                                                  ctypes.byref(res)), rows_out, REGION_JOINT_DTYPE)
    _check(lib, rc)
    return (rows, shapes, res) if want_shapes else (rows, res)


# ---- region components -----------------------------------------------------------------------------
def default_component_params(**overrides):
    p = ComponentParams()
    load_library().f3ds_default_component_params(ctypes.byref(p))
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


def region_components_host(depth, labels, n_regions, fmt, depth_tol=0.05, min_pixels=1, rows_out=None):
    """f3ds_region_components_host: (comp_labels, rows, RegionComponentsResult) -- the connected components (4-connectivity) of the label image: two
    neighbouring labelled pixels belong together iff their labels are equal and their depths are close (|za - zb| <= depth_tol * min(za, zb); depth_tol may be
    inf).  comp_labels is a (height, width) uint32 image of component numbers (0xFFFFFFFF where the pixel is not labelled or its component has fewer than
    ``min_pixels`` pixels), numbered in raster order of their first pixels; rows holds one REGION_COMPONENT_DTYPE row per component: the region it came from,
    its first pixel and its size.  Host arithmetic only: what Context.region_components computes on the device, bit for bit."""
    lib = load_library()
    f, d, _, lab = _region_inputs(fmt, depth, labels, None)
    prm, res = ComponentParams(float(depth_tol), int(min_pixels)), RegionComponentsResult()
    comp = np.empty((int(fmt.height), int(fmt.width)), np.uint32)
    rc, rows = _contact_rows(lambda ptr, cap, n_out: lib.f3ds_region_components_host(ctypes.byref(f), d.ctypes.data, lab.ctypes.data, int(n_regions), ctypes.byref(prm),
                                                                                      comp.ctypes.data, ptr, cap, n_out, ctypes.byref(res)), rows_out, REGION_COMPONENT_DTYPE)
    _check(lib, rc)
    return comp, rows, res


# ---- device context ------------------------------------------------------------------------------
def _lone(lib, answer, rows_out=None, count=None):
    """What a lone region call answers, from its batch of one frame (the C entry points are that too): the frame's status raised as the lone call's return
    code, else the frame's tuple.  count: the result field with the row count of a call whose rows the device counts."""
    frames, status = answer
    rc = int(status[0])
    if rc == 0 and count and isinstance(rows_out, np.ndarray) and getattr(frames[0][-1], count) > len(rows_out):      # (an empty buffer is a NULL pointer: the call only counted)
        rc = ERR_CAPACITY
    _check(lib, rc)
    return frames[0]


def _one_second(out):
    """the optional second output of a lone call (None / False, True, or a buffer) as its batch of one takes it"""
    return out if out is None or out is True or out is False else [out]


class Context(_Handle):
    """One (device, stream) pair with its grow-only scratch.  Not thread-safe; one per GPU/stream."""

    _destroy = "f3ds_destroy"

    def __init__(self, device=0):
        self.lib = load_library()
        h = ctypes.c_void_p()
        _check(self.lib, self.lib.f3ds_create(device, ctypes.byref(h)))
        self.handle = h
        self.device = device
        self.result = Result()
        self._n = 0

    def _get(self, what, outs, *lead, tail=()):
        """the arrays of f3ds_get_<what> (see _two_call)"""
        return _two_call(self.lib, getattr(self.lib, "f3ds_get_" + what), [self.handle, *lead], outs, tail)

    def set_stream(self, hip_stream_ptr):
        _check(self.lib, self.lib.f3ds_set_stream(self.handle, ctypes.c_void_p(hip_stream_ptr)))

    def segment(self, points, params, labels_out=None, n=None, on_device=False):
        """points: (N,4) float32 ndarray (host) or a device pointer (int) with ``n`` given and
        ``on_device=True``.  Returns the per-point labels (ndarray; ``labels_out`` itself when a host array is given) or writes
        them to the device pointer ``labels_out``."""
        if on_device:
            ptr, count = ctypes.c_void_p(int(points)), int(n)
            out_ptr = ctypes.c_void_p(int(labels_out)) if labels_out is not None else None
            _check(self.lib, self.lib.f3ds_segment(self.handle, ptr, count, 1, ctypes.byref(params), out_ptr, 1, ctypes.byref(self.result)))
            self._n = count
            return None
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        labels = _label_buffer(labels_out, len(pts), "point")      # (the caller's own buffer, reused from call to call: a fresh 80 MB array for a 20M-point scene is 20 000 page faults inside the download)
        _check(self.lib, self.lib.f3ds_segment(self.handle, pts.ctypes.data, len(pts), 0, ctypes.byref(params), labels.ctypes.data, 0,
                                               ctypes.byref(self.result)))
        self._n = len(pts)
        return labels

    def segment_rgbd(self, depth, color, fmt, params, labels_out=None, on_device=False):
        """f3ds_segment_rgbd: segment() on the records deproject(fmt, depth, color) gives, built on the device from the two images.
        depth: (height, width) uint16 / float32, color: (height, width, 3 | 4) uint8 or (height, width) uint32 as ``fmt`` says (rows may be
        strided), or device pointers (ints, the pitches of ``fmt`` apply) with ``on_device=True``; labels as in segment()."""
        n = int(fmt.width) * int(fmt.height)
        if on_device:
            out_ptr = ctypes.c_void_p(int(labels_out)) if labels_out is not None else None
            _check(self.lib, self.lib.f3ds_segment_rgbd(self.handle, ctypes.byref(fmt), ctypes.c_void_p(int(depth)), ctypes.c_void_p(int(color)), 1, ctypes.byref(params),
                                                        out_ptr, 1, ctypes.byref(self.result)))
            self._n = n
            return None
        f, d, c = _rgbd_images(fmt, depth, color)
        labels = _label_buffer(labels_out, n, "pixel")
        _check(self.lib, self.lib.f3ds_segment_rgbd(self.handle, ctypes.byref(f), d.ctypes.data, c.ctypes.data, 0, ctypes.byref(params), labels.ctypes.data, 0,
                                                    ctypes.byref(self.result)))
        self._n = n
        return labels

    def region_table(self, depth, labels, n_regions, fmt, color=None, rows_out=None, on_device=False):
        """f3ds_region_table: (rows, RegionTableResult) -- one REGION_ROW_DTYPE row per region of a label image of the frame (what segment_rgbd wrote, a level
        of labels_at_thresholds, ...), computed on the device in one read of the images; row i is region i, so its track id is ``Tracker.ids()[i]``.  depth,
        color, labels as in segment_rgbd / Tracker.update (color may be None: mean_rgb is then 0), or device pointers (ints, the pitches of ``fmt`` apply) with
        ``on_device=True``: ``rows_out`` is then a device pointer to n_regions rows and the rows returned are None.  Leaves the context's frame as it is."""
        return _lone(self.lib, region_table_batch([self], [depth], [labels], [n_regions], fmt, [color], [rows_out], on_device))

    def region_contacts(self, depth, labels, n_regions, fmt, depth_tol=0.05, rows_out=None, on_device=False):
        """f3ds_region_contacts: (rows, RegionContactsResult) -- what region_contacts_host returns, computed on the device; a and b index the rows of
        region_table and ``Tracker.ids()``.  depth and labels as in region_table, or device pointers (ints, the depth pitch of ``fmt`` applies) with
        ``on_device=True``: ``rows_out`` is then ``(device pointer, capacity in rows)`` or None (count only), the rows returned are None and
        ``result.n_contacts`` says how many were written (CapacityError, and none written, when there are more than the capacity).  With host arrays
        ``rows_out`` may be a REGION_CONTACT_DTYPE array to fill (the rows returned are a view of it); without it a buffer that turns out too small is grown
        from the count and the call repeated: one device pass when it suffices.  Leaves the context's frame as it is."""
        return _lone(self.lib, region_contacts_batch([self], [depth], [labels], [n_regions], fmt, depth_tol, [rows_out], on_device), rows_out, "n_contacts")

    def region_shapes(self, depth, labels, n_regions, fmt, rows_out=None, on_device=False):
        """f3ds_region_shapes: (rows, RegionShapesResult) -- what region_shapes_host returns, computed on the device in one read of the depth image and the
        labels; row i is region i, the row i of region_table and ``Tracker.ids()[i]``.  depth and labels as in region_table, or device pointers (ints, the depth
        pitch of ``fmt`` applies) with ``on_device=True``: ``rows_out`` is then a device pointer to n_regions rows and the rows returned are None.  With host
        arrays ``rows_out`` may be a REGION_SHAPE_DTYPE array to fill.  Leaves the context's frame as it is."""
        return _lone(self.lib, region_shapes_batch([self], [depth], [labels], [n_regions], fmt, [rows_out], on_device))

    def region_boxes(self, depth, labels, n_regions, fmt, plane_tol=0.01, rows_out=None, shapes_out=None, on_device=False):
        """f3ds_region_boxes: (rows, RegionBoxesResult) -- what region_boxes_host returns, computed on the device in two reads of the depth image and the
        labels with one wait; row i is region i, the row i of region_table and region_shapes.  With ``shapes_out`` the shape rows come too and the answer is
        (rows, shapes, RegionBoxesResult): ``True`` for a new REGION_SHAPE_DTYPE array, or such an array to fill.  depth and labels as in region_table, or
        device pointers (ints, the depth pitch of ``fmt`` applies) with ``on_device=True``: ``rows_out`` and ``shapes_out`` are then device pointers to
        n_regions rows each (``shapes_out`` may be None) and the rows returned are None.  With host arrays ``rows_out`` may be a REGION_BOX_DTYPE array to
        fill.  Leaves the context's frame as it is."""
        return _lone(self.lib, region_boxes_batch([self], [depth], [labels], [n_regions], fmt, plane_tol, [rows_out], _one_second(shapes_out), on_device))

    def cloud_regions(self, points, labels, n_regions, params=None, rows_out=None, boxes_out=None, n=None, on_device=False):
        """f3ds_cloud_regions: (rows, CloudRegionsResult) -- what cloud_regions_host returns, computed on the device with one wait.  points: (n, 4) float32
        records, or None for the records the context's last segment call ran on (LogicError when they were the caller's device buffer).  With ``boxes_out`` the
        boxes come too and the answer is (rows, boxes, CloudRegionsResult): ``True`` for a new REGION_BOX_DTYPE array, or such an array to fill.  With
        ``on_device=True`` points (or None) and labels are device pointers (ints or torch tensors), ``n`` the point count, ``rows_out`` and ``boxes_out`` device
        pointers to n_regions rows each (``boxes_out`` may be None) and the rows returned are None.  Leaves the context's frame as it is."""
        if on_device and n is None:
            raise ValueError("on_device needs the point count n")
        return _lone(self.lib, cloud_regions_batch([self], [points], [labels], [n_regions], params, [rows_out], _one_second(boxes_out), None if n is None else [n], on_device))

    def cloud_path(self):
        """F3DS_DBG_CLOUD_PATH: how the context's last cloud_regions call walked its points -- "direct", "ordered", or None before any."""
        w = np.zeros(1, np.uint32)
        _check(self.lib, self.lib.f3ds_get_debug(self.handle, DBG_CLOUD_PATH, w.ctypes.data, 4, None))
        return {1: "direct", 2: "ordered"}.get(int(w[0]))

    def region_joints(self, depth, labels, n_regions, fmt, params=None, rows_out=None, shapes_out=None, on_device=False):
        """f3ds_region_joints: (rows, RegionJointsResult) -- what region_joints_host returns, computed on the device with one wait; a and b index the rows of
        region_table and region_shapes.  With ``shapes_out`` the shape rows come too and the answer is (rows, shapes, RegionJointsResult): ``True`` for a new
        REGION_SHAPE_DTYPE array, or such an array to fill.  depth and labels as in region_table, or device pointers (ints, the depth pitch of ``fmt`` applies)
        with ``on_device=True``: ``rows_out`` is then ``(device pointer, capacity in rows)`` or None (count only), ``shapes_out`` a device pointer to n_regions
        rows or None, the rows returned are None and ``result.n_joints`` says how many were written (CapacityError, and none written, when there are more than
        the capacity).  With host arrays ``rows_out`` may be a REGION_JOINT_DTYPE array to fill; without it a buffer that turns out too small is grown from the
        count and the call repeated.  Leaves the context's frame as it is."""
        return _lone(self.lib, region_joints_batch([self], [depth], [labels], [n_regions], fmt, params, [rows_out], _one_second(shapes_out), on_device), rows_out, "n_joints")

    def region_components(self, depth, labels, n_regions, fmt, depth_tol=0.05, min_pixels=1, rows_out=None, comp_out=None, on_device=False):
        """f3ds_region_components: (comp_labels, rows, RegionComponentsResult) -- what region_components_host returns, computed on the device.  The image is a
        label image again: region_table, region_contacts, region_shapes and Tracker.update run on it with ``n_regions = result.n_components``.  depth and
        labels as in region_table, or device pointers (ints, the depth pitch of ``fmt`` applies) with ``on_device=True``: ``comp_out`` is then a device pointer to
        width * height words, ``rows_out`` is ``(device pointer, capacity in rows)`` or None (no rows), image and rows returned are None and
        ``result.n_components`` says how many rows were written (CapacityError, and none written, when there are more than the capacity).  With host arrays
        ``rows_out`` may be a REGION_COMPONENT_DTYPE array to fill; without it a buffer that turns out too small is grown from the count and the call
        repeated: one device pass when it suffices.  Leaves the context's frame as it is."""
        return _lone(self.lib, region_components_batch([self], [depth], [labels], [n_regions], fmt, depth_tol, min_pixels, [rows_out], [comp_out], on_device), rows_out,
                     "n_components")

    def points(self):
        """f3ds_get_points: the (N, 4) float32 records the last segment call ran on, when the context holds them (segment_rgbd, or segment
        with host points); LogicError when they were the caller's device buffer or nothing has run."""
        return self._get("points", [(np.float32, (4,))], tail=[0])[0]

    def recluster(self, params):
        labels = np.empty(int(self.result.n_points) or self._n, np.uint32)      # f3ds_recluster writes one label per point of the frame
        _check(self.lib, self.lib.f3ds_recluster(self.handle, ctypes.byref(params), labels.ctypes.data, 0, ctypes.byref(self.result)))
        return labels

    def _level_count(self):
        return int(self.result.n_points) or self._n

    def labels_at_thresholds(self, thresholds, out=None, on_device=False):
        """f3ds_labels_at_thresholds: the labels of every threshold t <= T of the last cluster run (segment / recluster /
        cluster_supervoxels at T) from that run's merge log, without merging again.  Returns (labels, n_regions): labels is a
        (k, n) uint32 array whose row l equals recluster(threshold=t_l), n_regions a (k,) uint32 array.  ``on_device``: ``out`` is a
        device buffer of k * n uint32 (a torch tensor or a pointer) written in place, and labels is ``out``."""
        t = np.ascontiguousarray(np.atleast_1d(np.asarray(thresholds, np.float32)).ravel())
        k, n = len(t), self._level_count()
        nreg = np.zeros(max(k, 1), np.uint32)
        if on_device:
            ptr = _device_ptr(out)
            labels = out
        else:
            labels = np.empty((k, n), np.uint32) if out is None else out
            if not (isinstance(labels, np.ndarray) and labels.dtype == np.uint32 and labels.flags.c_contiguous and labels.size == k * n):
                raise ValueError("out must be a contiguous uint32 array of k * n = %d entries" % (k * n))
            ptr = labels.ctypes.data
        _check(self.lib, self.lib.f3ds_labels_at_thresholds(self.handle, t.ctypes.data, k, ptr, 1 if on_device else 0, nreg.ctypes.data))
        return labels, nreg[:k]

    def evaluate_levels(self, truth, thresholds, on_device=False):
        """f3ds_evaluate_levels: the scores of recluster(threshold=t_l) + evaluate(truth) for every threshold t_l <= T of the last
        cluster run, on the device, from that run's merge log.  Returns (list of k Performance, (k,) uint32 region counts).
        ``on_device``: ``truth`` is a device buffer of n uint32 labels (a torch tensor or a pointer)."""
        scores, nreg = evaluate_levels_batch([self], [truth], thresholds, on_device)
        return scores[0], nreg[0]

    def merge_tree(self):
        """f3ds_get_merge_tree: the merges of the last cluster run in the order performed, as (survivor, absorbed, weight) arrays of
        supervoxel labels (the caller's keys after cluster_supervoxels) and float32 weights."""
        return tuple(self._get("merge_tree", [_U32, _U32, _F32]))

    def evaluate(self, truth_point_labels):
        """Scores of the current segmentation against per-point ground-truth labels (Testing::eval_performance)."""
        t = np.ascontiguousarray(truth_point_labels, np.uint32)
        if len(t) != self._n:
            raise ValueError("one ground-truth label per input point is required")
        out = Performance()
        _check(self.lib, self.lib.f3ds_evaluate(self.handle, t.ctypes.data, ctypes.byref(out)))
        return out

    def auto_threshold(self, params, truth_point_labels, start=0.8, end=1.0, step=0.005):
        """all_thresh + best_thresh; returns (best threshold, best scores, {threshold: scores}, point labels)."""
        t = np.ascontiguousarray(truth_point_labels, np.uint32)
        if len(t) != self._n:
            raise ValueError("one ground-truth label per input point is required")
        cap = 4096
        ts = np.zeros(cap, np.float32); ps = (Performance * cap)()
        n = ctypes.c_size_t(); bt = ctypes.c_float(); bp = Performance()
        labels = np.empty(self._n, np.uint32)
        _check(self.lib, self.lib.f3ds_auto_threshold(self.handle, ctypes.byref(params), t.ctypes.data, start, end, step, ts.ctypes.data, ps, cap,
                                                      ctypes.byref(n), ctypes.byref(bt), ctypes.byref(bp), labels.ctypes.data, 0, ctypes.byref(self.result)))
        m = min(n.value, cap)
        return bt.value, bp, {float(ts[i]): ps[i].as_dict() for i in range(m)}, labels

    def voxel_centroid_cloud(self):
        """getVoxelCentroidCloud / getLabeledVoxelCloud: (xyz, rgba, supervoxel label) per voxel in leaf order."""
        return tuple(self._get("voxel_centroid_cloud", [_XYZ, _U32, _U32]))

    def supervoxels(self):
        """The supervoxel_clusters map: dict of arrays label, xyz, rgb, normal, n_voxels (ascending label)."""
        return dict(zip(("label", "xyz", "rgb", "normal", "n_voxels"), self._get("supervoxels", [_U32, _XYZ, _XYZ, _XYZ, _U32])))

    def refine_supervoxels(self, num_itr):
        """refineSupervoxels(num_itr): dict with per-voxel ``voxel_label`` / ``voxel_normal`` (leaf order) and the refined
        supervoxel map ``label, xyz, rgb, normal, n_voxels``.  The frame's own supervoxels and clustering are untouched."""
        _check(self.lib, self.lib.f3ds_refine_supervoxels(self.handle, int(num_itr)))
        return dict(zip(("voxel_label", "voxel_normal", "label", "xyz", "rgb", "normal", "n_voxels"),
                        self._get("refined_voxels", [_U32, _XYZ]) + self._get("refined_supervoxels", [_U32, _XYZ, _XYZ, _XYZ, _U32])))

    def supervoxel_adjacency(self):
        """getSupervoxelAdjacency after clear_adjacency: (E, 2) array of label pairs a < b, sorted."""
        return self._get("supervoxel_adjacency", [_PAIR])[0]

    def region_adjacency(self):
        """get_currentstate().second after cluster(): (K, 2) array of surviving supervoxel labels a < b, sorted."""
        return self._get("region_adjacency", [_PAIR])[0]

    def cluster_supervoxels(self, sv, adjacency_pairs, params):
        """f3ds_cluster_supervoxels: Clustering::set_initialstate(segm, adj) + cluster(threshold) on caller-supplied supervoxels.
        ``sv``: dict of arrays label, voxel_offset, voxel_xyz, voxel_rgba, centroid_xyz, normal (see pack_supervoxels);
        ``adjacency_pairs``: (P, 2) uint32 in multimap iteration order.  Returns (region_of_sv, voxel_labels)."""
        a = {k: np.ascontiguousarray(sv[k], np.float32 if k in ("voxel_xyz", "centroid_xyz", "normal") else np.uint32) for k in
             ("label", "voxel_offset", "voxel_xyz", "voxel_rgba", "centroid_xyz", "normal")}
        S = len(a["label"])
        # the C entry reads voxel_offset[0..S], voxel_offset[S] voxels and S centroid / normal rows through raw pointers: arrays that disagree with each other
        # would be read past their end (pack_supervoxels' output is consistent; any other dict is checked here)
        if a["voxel_offset"].shape != (S + 1,):
            raise ValueError("voxel_offset must hold n_supervoxels + 1 = %d entries, has shape %s" % (S + 1, a["voxel_offset"].shape))
        nvox = int(a["voxel_offset"][S])
        if a["voxel_xyz"].size != 3 * nvox or a["voxel_rgba"].size != nvox:
            raise ValueError("voxel_xyz / voxel_rgba must hold voxel_offset[-1] = %d voxels (have %d / %d)" % (nvox, a["voxel_xyz"].size // 3, a["voxel_rgba"].size))
        if a["centroid_xyz"].size != 3 * S or a["normal"].size != 3 * S:
            raise ValueError("centroid_xyz and normal must have shape (%d, 3)" % S)
        st = SupervoxelSet(S, *[a[k].ctypes.data for k in ("label", "voxel_offset", "voxel_xyz", "voxel_rgba", "centroid_xyz", "normal")])
        pairs = np.ascontiguousarray(adjacency_pairs, np.uint32).reshape(-1, 2)
        region = np.zeros(S, np.uint32); vlab = np.zeros(nvox, np.uint32)
        _check(self.lib, self.lib.f3ds_cluster_supervoxels(self.handle, ctypes.byref(st), pairs.ctypes.data, len(pairs), ctypes.byref(params), region.ctypes.data,
                                                           vlab.ctypes.data, ctypes.byref(self.result)))
        self._n = nvox
        return region, vlab

    def regions(self):
        """get_currentstate().first: dict of arrays label, n_voxels, xyz (centroid_), normal (normal_), rgb (mean_color) per merged region, ascending key."""
        return dict(zip(("label", "n_voxels", "xyz", "normal", "rgb"), self._get("regions", [_U32, _U32, _XYZ, _XYZ, _XYZ])))

    def region_voxels(self):
        """The regions' voxels_ clouds concatenated in the order of regions(): (xyz, rgba, voxel index)."""
        return tuple(self._get("region_voxels", [_XYZ, _U32, _U32]))

    def voxel_cloud(self):
        return tuple(self._get("voxel_cloud", [_XYZ, _U32, _U32]))

    def merge_layout(self):
        """(waves per frame, per-edge arrays in LDS) of the merge kernel the last cluster stage ran; (0, 0) = d_merge (F3DS_DBG_MERGE_LAYOUT)."""
        nb = ctypes.c_size_t(); buf = np.zeros(2, np.uint32)
        _check(self.lib, self.lib.f3ds_get_debug(self.handle, 20, buf.ctypes.data, 8, ctypes.byref(nb)))
        return int(buf[0]), int(buf[1])

    def stage0_path(self):
        """'tiles' or 'sort': how the last frame was voxelised (F3DS_DBG_STAGE0_PATH)."""
        nb = ctypes.c_size_t(); buf = np.zeros(1, np.uint32)
        _check(self.lib, self.lib.f3ds_get_debug(self.handle, 23, buf.ctypes.data, 4, ctypes.byref(nb)))
        return "tiles" if buf[0] else "sort"

    def launch_shape(self):
        """(workgroups per frame a streaming kernel got at most, ... a gathering kernel got at most, frames of the call) of the last call that ran
        kernels for this context (F3DS_DBG_LAUNCH_SHAPE).  (2048, 2048, 1) for a lone frame unless the development switch F3DS_GRID_CAP narrows the launches."""
        nb = ctypes.c_size_t(); buf = np.zeros(3, np.uint32)
        _check(self.lib, self.lib.f3ds_get_debug(self.handle, DBG_INFO["LAUNCH_SHAPE"], buf.ctypes.data, 12, ctypes.byref(nb)))
        return tuple(int(x) for x in buf)

    def sweep_stats(self):
        """(full, incremental, fallback, skipped) sweeps of the last run of label-propagation sweeps (F3DS_DBG_SWEEP_STATS)."""
        nb = ctypes.c_size_t(); buf = np.zeros(4, np.uint32)
        _check(self.lib, self.lib.f3ds_get_debug(self.handle, 22, buf.ctypes.data, 16, ctypes.byref(nb)))
        return tuple(int(x) for x in buf)

    def tile_list_lengths(self):
        """Length of every 128-voxel tile's one-ring list; 0xFFFFFFFF = the tile overflowed the LDS tables (F3DS_DBG_TILE_LIST_LEN)."""
        return self._get("debug", [(np.uint8, ())], DBG_INFO["TILE_LIST_LEN"])[0].view(np.uint32)

    def debug(self, name):
        return self._get("debug", [(np.uint8, ())], DBG[name])[0].view(DBG_DTYPE[name])


class FrameStream(_Handle):
    """Frame pipeline (f3ds_stream_*): frames in from host memory, per-point labels out in submission order, up to
    ``depth`` frames in flight on ``groups`` host threads.  ``submit`` returns False instead of blocking when the
    pipeline is full; ``next`` returns (tag, labels, Result) of the oldest frame, None when nothing is in flight."""

    _destroy = "f3ds_stream_destroy"

    def __init__(self, device=0, depth=8, groups=0):
        self.lib = load_library()
        h = ctypes.c_void_p()
        _check(self.lib, self.lib.f3ds_stream_create(device, depth, groups, ctypes.byref(h)))
        self.handle = h
        self.depth = depth

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def pending(self):
        return self.lib.f3ds_stream_pending(self.handle)

    def buffer(self, n):
        """(n,4) float32 view of the pinned input buffer the next submit uses, or None when the pipeline is full."""
        p = ctypes.c_void_p()
        rc = self.lib.f3ds_stream_buffer(self.handle, n, ctypes.byref(p))
        if rc == ERR_BUSY:
            return None
        _check(self.lib, rc)
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_float)), shape=(max(n, 1), 4))[:n]

    def submit(self, points, params, tag=0):
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        rc = self.lib.f3ds_stream_submit(self.handle, pts.ctypes.data, len(pts), ctypes.byref(params), tag)
        if rc == ERR_BUSY:
            return False
        _check(self.lib, rc)
        return True

    def submit_rgbd(self, depth, color, fmt, params, tag=0):
        """Queue an RGB-D frame (host images as Context.segment_rgbd takes them); its width * height labels come out of next() / peek() in
        submission order, among those of submit()."""
        f, d, c = _rgbd_images(fmt, depth, color)
        rc = self.lib.f3ds_stream_submit_rgbd(self.handle, ctypes.byref(f), d.ctypes.data, c.ctypes.data, ctypes.byref(params), tag)
        if rc == ERR_BUSY:
            return False
        _check(self.lib, rc)
        return True

    def next(self, wait=True):
        n = ctypes.c_size_t(); tag = ctypes.c_uint64(); res = Result()
        probe = np.empty(1, np.uint32)
        rc = self.lib.f3ds_stream_next(self.handle, probe.ctypes.data, 0, ctypes.byref(n), ctypes.byref(tag), ctypes.byref(res), 1 if wait else 0)
        if rc in (ERR_EMPTY, ERR_BUSY):
            return None
        labels = np.empty(n.value, np.uint32)
        if rc == ERR_CAPACITY:                              # the frame is done and still there: now with room for its labels
            rc = self.lib.f3ds_stream_next(self.handle, labels.ctypes.data, len(labels), ctypes.byref(n), ctypes.byref(tag), ctypes.byref(res), 1)
        _check(self.lib, rc)
        return tag.value, labels, res

    def peek(self, wait=True):
        """(tag, labels, Result) of the oldest frame without copying: ``labels`` is a view of the slot's pinned buffer,
        valid until ``drop()``.  None when nothing is in flight (or, with wait=False, not done yet)."""
        n = ctypes.c_size_t(); tag = ctypes.c_uint64(); res = Result(); p = ctypes.c_void_p()
        rc = self.lib.f3ds_stream_peek(self.handle, ctypes.byref(p), ctypes.byref(n), ctypes.byref(tag), ctypes.byref(res), 1 if wait else 0)
        if rc in (ERR_EMPTY, ERR_BUSY):
            return None
        _check(self.lib, rc)
        lab = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint32)), shape=(max(n.value, 1),))[:n.value]
        return tag.value, lab, res

    def drop(self):
        """Take the oldest (finished) frame out of the pipeline without copying its labels."""
        rc = self.lib.f3ds_stream_next(self.handle, None, 0, None, None, None, 1)
        if rc != ERR_EMPTY:
            _check(self.lib, rc)

    def run(self, frames, params):
        """Generator: feed an iterable of (N,4) frames, yield (index, labels, Result) in order."""
        i = 0
        for pts in frames:
            while not self.submit(pts, params, i):
                yield self.next()
            i += 1
        while self.pending():
            yield self.next()


class MultiGpu(_Handle):
    """f3ds_multi_*: a batch of independent frames sharded over the GPUs of one node from ONE process (frame i on
    devices[i mod G], one host thread per GPU inside the library), per-point labels gathered on devices[0] over RCCL and
    returned as host arrays.  The torch.distributed form of the same partitioning (one process per GPU) is batch.py."""

    _destroy = "f3ds_multi_destroy"

    def __init__(self, devices=None, n_devices=None, max_frames_per_device=8):
        self.lib = load_library()
        if devices is not None:
            arr = (ctypes.c_int * len(devices))(*devices); n = len(devices)
        else:
            arr = None; n = int(n_devices or 1)
        h = ctypes.c_void_p()
        rc = self.lib.f3ds_multi_create(arr, n, int(max_frames_per_device), ctypes.byref(h))
        if rc:
            raise F3dsError(rc, self.lib.f3ds_strerror(rc).decode() + " " + self.lib.f3ds_multi_last_error().decode())
        self.handle = h

    def devices(self):
        return self.lib.f3ds_multi_devices(self.handle)

    def device_of_frame(self, frame):
        return self.lib.f3ds_multi_device_of_frame(self.handle, frame)

    def _error(self, rc):
        return F3dsError(rc, self.lib.f3ds_strerror(rc).decode() + " " + self.lib.f3ds_multi_last_error().decode() + " " + self.lib.f3ds_last_hip_error().decode())

    def reserve(self, max_points_per_frame):
        """Allocate the label blocks for full batches of frames of up to that many points now, not inside the first batches."""
        rc = self.lib.f3ds_multi_reserve(self.handle, int(max_points_per_frame))
        if rc:
            raise self._error(rc)

    def submit(self, frames, params):
        """Queue a batch (list of (N_i, 4) float32 arrays) and return a ticket: the GPUs compute it while the batch before it is
        gathered and copied out.  At most two batches are in flight (F3dsError ERR_BUSY: collect the older one first)."""
        k = len(frames)
        vp = ctypes.c_void_p
        arrs = [np.ascontiguousarray(f, np.float32).reshape(-1, 4) for f in frames]
        out = [np.empty(len(a), np.uint32) for a in arrs]
        pp = (vp * max(k, 1))(*[vp(a.ctypes.data) for a in arrs]); lp = (vp * max(k, 1))(*[vp(o.ctypes.data) for o in out])
        cnt = (ctypes.c_size_t * max(k, 1))(*[len(a) for a in arrs])
        results = (Result * max(k, 1))()
        prm = params.copy()
        t = ctypes.c_int(-1)
        rc = self.lib.f3ds_multi_submit(self.handle, pp, cnt, k, ctypes.byref(prm), lp, results, ctypes.byref(t))
        if rc:
            raise self._error(rc)
        if not hasattr(self, "_inflight"):
            self._inflight = {}
        self._inflight[t.value] = (arrs, out, results, k)      # the buffers stay alive until the batch is collected
        return t.value

    def collect(self, ticket):
        """Wait for a submitted batch.  Returns (list of label arrays, list of Result)."""
        arrs, out, results, k = self._inflight.pop(ticket)
        rc = self.lib.f3ds_multi_collect(self.handle, int(ticket))
        if rc:
            raise self._error(rc)
        return out, [results[i] for i in range(k)]

    def segment(self, frames, params):
        """frames: list of (N_i, 4) float32 arrays.  Returns (list of label arrays, list of Result)."""
        if not frames:
            return [], []
        return self.collect(self.submit(frames, params))


def segment_batch(ctxs, points, params, labels_out=None, n=None, on_device=False, raw_host=False):
    """Segment len(ctxs) independent frames at once (one context per frame, all on one GPU).
    Host mode: points = list of (N_i,4) float32 arrays, returns a list of label arrays.
    Device mode (on_device): points / labels_out = lists of device pointers, n = list of point counts.
    raw_host: the same with host pointers (e.g. pinned buffers of the caller): PCIe both ways inside the call."""
    lib = load_library()
    k = len(ctxs)
    vp = ctypes.c_void_p
    handles = (vp * k)(*[c.handle for c in ctxs])
    results = (Result * k)()
    if on_device or raw_host:
        where = 1 if on_device else 0
        pp = (vp * k)(*[vp(int(p)) for p in points]); lp = (vp * k)(*[vp(int(p)) for p in labels_out])
        cnt = (ctypes.c_size_t * k)(*[int(x) for x in n])
        _check(lib, lib.f3ds_segment_batch(handles, k, pp, cnt, where, ctypes.byref(params), lp, where, results))
        for c, x in zip(ctxs, n):
            c._n = int(x)
        out = None
    else:
        arrs = [np.ascontiguousarray(p, np.float32).reshape(-1, 4) for p in points]
        out = [np.empty(len(a), np.uint32) for a in arrs]
        pp = (vp * k)(*[vp(a.ctypes.data) for a in arrs]); lp = (vp * k)(*[vp(o.ctypes.data) for o in out])
        cnt = (ctypes.c_size_t * k)(*[len(a) for a in arrs])
        _check(lib, lib.f3ds_segment_batch(handles, k, pp, cnt, 0, ctypes.byref(params), lp, 0, results))
        for c, a in zip(ctxs, arrs):
            c._n = len(a)
    for c, r in zip(ctxs, results):
        ctypes.memmove(ctypes.byref(c.result), ctypes.byref(r), ctypes.sizeof(Result))
    return out


def segment_rgbd_batch(ctxs, depths, colors, fmt, params, labels_out=None, on_device=False, raw_host=False):
    """f3ds_segment_rgbd_batch: Context.segment_rgbd for len(ctxs) frames of ONE format at once (one context per frame, all on one GPU).
    Host mode: depths / colors = lists of arrays with the same row strides, returns a list of label arrays.  on_device / raw_host: lists of
    device / host pointers (ints) and ``labels_out`` likewise; the pitches of ``fmt`` apply."""
    lib = load_library()
    k = len(ctxs)
    vp = ctypes.c_void_p
    handles = (vp * k)(*[c.handle for c in ctxs])
    results = (Result * k)()
    n = int(fmt.width) * int(fmt.height)
    if on_device or raw_host:
        where = 1 if on_device else 0
        dp = (vp * k)(*[vp(int(p)) for p in depths]); cp = (vp * k)(*[vp(int(p)) for p in colors]); lp = (vp * k)(*[vp(int(p)) for p in labels_out])
        _check(lib, lib.f3ds_segment_rgbd_batch(handles, k, ctypes.byref(fmt), dp, cp, where, ctypes.byref(params), lp, where, results))
        out = None
    else:
        imgs = [_rgbd_images(fmt, d, c) for d, c in zip(depths, colors)]
        f = imgs[0][0]
        for g, d, c in imgs[1:]:
            if (g.depth_pitch, g.color_pitch) != (f.depth_pitch, f.color_pitch):
                raise ValueError("the images of a batch must share their row strides (one f3ds_rgbd_format for the batch)")
        out = [np.empty(n, np.uint32) for _ in imgs]
        dp = (vp * k)(*[vp(d.ctypes.data) for _, d, _c in imgs]); cp = (vp * k)(*[vp(c.ctypes.data) for _, _d, c in imgs]); lp = (vp * k)(*[vp(o.ctypes.data) for o in out])
        _check(lib, lib.f3ds_segment_rgbd_batch(handles, k, ctypes.byref(f), dp, cp, 0, ctypes.byref(params), lp, 0, results))
    for c, r in zip(ctxs, results):
        c._n = n
        ctypes.memmove(ctypes.byref(c.result), ctypes.byref(r), ctypes.sizeof(Result))
    return out


def _device_ptr(buf):
    """device address of a torch tensor / an integer pointer"""
    if buf is None:
        raise ValueError("on_device needs a device output buffer")
    return ctypes.c_void_p(buf.data_ptr() if hasattr(buf, "data_ptr") else int(buf))


def labels_at_thresholds_batch(ctxs, thresholds, out=None, on_device=False):
    """f3ds_labels_at_thresholds_batch: Context.labels_at_thresholds for every context at once (one GPU, one dispatch per kernel).
    Returns (list of (k, n_i) uint32 label arrays, (len(ctxs), k) uint32 region counts).  ``on_device``: ``out`` is a list of device
    buffers (torch tensors or pointers) of k * n_i uint32 each, written in place and returned."""
    lib = load_library()
    t = np.ascontiguousarray(np.atleast_1d(np.asarray(thresholds, np.float32)).ravel())
    k, m = len(t), len(ctxs)
    vp = ctypes.c_void_p
    handles = (vp * m)(*[c.handle for c in ctxs])
    if on_device:
        if out is None or len(out) != m:
            raise ValueError("on_device needs one device output buffer per context")
        labels = list(out)
        lp = (vp * m)(*[_device_ptr(o) for o in out])
    else:
        labels = [np.empty((k, c._level_count()), np.uint32) for c in ctxs] if out is None else list(out)
        for c, o in zip(ctxs, labels):
            if not (isinstance(o, np.ndarray) and o.dtype == np.uint32 and o.flags.c_contiguous and o.size == k * c._level_count()):
                raise ValueError("out[i] must be a contiguous uint32 array of k * n_i entries")
        lp = (vp * m)(*[vp(o.ctypes.data) for o in labels])
    nreg = np.zeros((max(m, 1), max(k, 1)), np.uint32)
    _check(lib, lib.f3ds_labels_at_thresholds_batch(handles, m, t.ctypes.data, k, lp, 1 if on_device else 0, nreg.ctypes.data))
    return labels, nreg[:m, :k]


def evaluate_levels_batch(ctxs, truths, thresholds, on_device=False):
    """f3ds_evaluate_levels_batch: Context.evaluate_levels for every context at once (one GPU, one dispatch per kernel for all frames
    and levels).  ``truths[i]``: the n_i ground-truth labels of ctxs[i] (device buffers with ``on_device``).  Returns (list of lists of k
    Performance, (len(ctxs), k) uint32 region counts)."""
    lib = load_library()
    t = np.ascontiguousarray(np.atleast_1d(np.asarray(thresholds, np.float32)).ravel())
    k, m = len(t), len(ctxs)
    if len(truths) != m:
        raise ValueError("one ground-truth label array per context is required")
    vp = ctypes.c_void_p
    handles = (vp * m)(*[c.handle for c in ctxs])
    if on_device:
        keep = list(truths)
        tp = (vp * m)(*[_device_ptr(x) for x in keep])
    else:
        keep = [np.ascontiguousarray(x, np.uint32) for x in truths]
        for c, x in zip(ctxs, keep):
            if c._n and len(x) != c._n:      # (a context that has not seen a frame yet is the library's to refuse: LogicError)
                raise ValueError("one ground-truth label per input point is required")
        tp = (vp * m)(*[vp(x.ctypes.data) for x in keep])
    ps = (Performance * (max(m, 1) * max(k, 1)))()
    nreg = np.zeros((max(m, 1), max(k, 1)), np.uint32)
    _check(lib, lib.f3ds_evaluate_levels_batch(handles, m, tp, 1 if on_device else 0, t.ctypes.data, k, ps, nreg.ctypes.data))
    return [[ps[i * k + l] for l in range(k)] for i in range(m)], nreg[:m, :k]


# ---- batch forms of the five region calls ----------------------------------------------------------
# One call for len(ctxs) frames of ONE format (one context per frame, all on one GPU): one dispatch per kernel, one wait.  Every function returns
# (frames, status): frames[i] is what the Context method of the same name returns for frame i, status an int32 array of the frames' outcomes (OK, ERR_ARG for a
# label >= n_regions[i], ERR_CAPACITY); the rows (and image) of a frame that failed are None, its result too after ERR_ARG.  An exception is raised, as by the
# Context methods, only when the call as a whole was refused.
_STATUS_UNSET = 1      # (no error code is positive: a status array that still holds this was not written, so the call as a whole was refused)


def _opt_ptr(p):
    return None if p is None else _device_ptr(p)


def _region_batch_inputs(ctxs, depths, labels, n_regions, fmt, colors, on_device):
    """(k, handles, format, depth / colour / label pointer arrays, region counts, status, what must stay alive) of a batch call"""
    k = len(ctxs)
    if k < 1:
        raise ValueError("a batch needs at least one context")
    for name, seq in (("depths", depths), ("labels", labels), ("n_regions", n_regions)):
        if len(seq) != k:
            raise ValueError("%s must hold one entry per context" % name)
    if colors is not None:
        if len(colors) != k:
            raise ValueError("colors must hold one entry per context")
        if all(c is None for c in colors):
            colors = None
        elif any(c is None for c in colors):
            raise ValueError("colors: an image for every frame or for none (one command sequence for the batch)")
    vp = ctypes.c_void_p
    handles = (vp * k)(*[c.handle for c in ctxs])
    nr = (ctypes.c_uint32 * k)(*[int(x) for x in n_regions])
    status = np.full(k, _STATUS_UNSET, np.int32)
    if on_device:
        f, keep = fmt, None
        dp = (vp * k)(*[_device_ptr(d) for d in depths]); lp = (vp * k)(*[_device_ptr(x) for x in labels])
        cp = None if colors is None else (vp * k)(*[_device_ptr(c) for c in colors])
    else:
        keep = [_region_inputs(fmt, d, lab, None if colors is None else colors[i]) for i, (d, lab) in enumerate(zip(depths, labels))]
        f = keep[0][0]
        for g in keep[1:]:
            if (g[0].depth_pitch, g[0].color_pitch) != (f.depth_pitch, f.color_pitch):
                raise ValueError("the images of a batch must share their row strides (one f3ds_rgbd_format for the batch)")
        dp = (vp * k)(*[vp(x[1].ctypes.data) for x in keep]); lp = (vp * k)(*[vp(x[3].ctypes.data) for x in keep])
        cp = None if colors is None else (vp * k)(*[vp(x[2].ctypes.data) for x in keep])
    return k, handles, f, dp, cp, lp, nr, status, keep


def _outs(seq, k, name):
    if seq is None:
        return [None] * k
    if len(seq) != k:
        raise ValueError("%s must hold one entry per context" % name)
    return list(seq)


def _batch_done(lib, rc, status):
    """raise iff the call as a whole was refused (or failed): the frames' statuses were not written then"""
    if rc != 0 and (status == _STATUS_UNSET).all():
        _check(lib, rc)
    return status


def _second_out(out, k, name, what, on_device, make_rows, nr, spare=None):
    """The optional second output of a batch call (the shape rows of the boxes and the joints, the boxes of the cloud rows).  ``out``: None / False, ``True``
    (host form: new arrays) or a list of buffers, for every frame or for none.  Returns (wanted?, the k arrays -- None without, or on the device --, the pointer
    array or None); the pointer of an array without rows is ``spare``'s, or NULL."""
    if out is None or out is False:
        return False, [None] * k, None
    outs = [None] * k if out is True else _outs(out, k, name)
    if out is not True and any(o is None for o in outs):
        raise ValueError("%s: a buffer for every frame or None (one command sequence for the batch)" % name)
    vp = ctypes.c_void_p
    if on_device:
        if out is True:
            raise ValueError("on_device needs device buffers for " + what)
        return True, [None] * k, (vp * k)(*[_opt_ptr(o) for o in outs])
    arrays = [make_rows(o, nr[i]) for i, o in enumerate(outs)]
    empty = None if spare is None else vp(spare.ctypes.data)
    return True, arrays, (vp * k)(*[vp(a.ctypes.data) if len(a) else empty for a in arrays])


def _fixed_rows_batch(fn, make_rows, res_type, ctxs, depths, labels, n_regions, fmt, colors, rows_out, on_device, lead=(), with_color=False):
    """the batch calls with one row per region (table, shapes): fn(handles, k, fmt, depth[, color], labels, n_regions, *lead, on_device, rows, on_device, results, status)"""
    lib = load_library()
    k, handles, f, dp, cp, lp, nr, status, keep = _region_batch_inputs(ctxs, depths, labels, n_regions, fmt, colors, on_device)
    vp = ctypes.c_void_p
    outs, results = _outs(rows_out, k, "rows_out"), (res_type * k)()
    if on_device:
        rows = [None] * k
        rp = (vp * k)(*[_opt_ptr(o) for o in outs])
    else:
        rows = [make_rows(o, nr[i]) for i, o in enumerate(outs)]
        rp = (vp * k)(*[vp(r.ctypes.data) if len(r) else None for r in rows])
    where = 1 if on_device else 0
    images = (dp, cp, lp) if with_color else (dp, lp)
    rc = fn(handles, k, ctypes.byref(f), *images, nr, *lead, where, rp, where, results, status.ctypes.data)
    _batch_done(lib, rc, status)
    return [(rows[i] if status[i] == 0 else None, results[i] if status[i] == 0 else None) for i in range(k)], status


def region_table_batch(ctxs, depths, labels, n_regions, fmt, colors=None, rows_out=None, on_device=False):
    """f3ds_region_table_batch: Context.region_table for every frame at once.  depths / labels / colors: lists of arrays, or of device pointers / torch tensors
    with ``on_device`` (``rows_out`` is then a list of device buffers); colors: an image for every frame, or None.  Returns ([(rows, RegionTableResult)], status)."""
    return _fixed_rows_batch(load_library().f3ds_region_table_batch, _region_rows, RegionTableResult, ctxs, depths, labels, n_regions, fmt, colors, rows_out, on_device,
                             with_color=True)


def region_shapes_batch(ctxs, depths, labels, n_regions, fmt, rows_out=None, on_device=False):
    """f3ds_region_shapes_batch: Context.region_shapes for every frame at once (lists as in region_table_batch).  Returns ([(rows, RegionShapesResult)], status)."""
    return _fixed_rows_batch(load_library().f3ds_region_shapes_batch, _shape_rows, RegionShapesResult, ctxs, depths, labels, n_regions, fmt, None, rows_out, on_device)


def region_boxes_batch(ctxs, depths, labels, n_regions, fmt, plane_tol=0.01, rows_out=None, shapes_out=None, on_device=False):
    """f3ds_region_boxes_batch: Context.region_boxes for every frame at once (lists as in region_table_batch).  ``shapes_out``: None, ``True`` (host form: new
    arrays) or a list of buffers, for every frame or for none.  Returns ([(rows, RegionBoxesResult)], status), or ([(rows, shapes, RegionBoxesResult)], status)
    with shapes."""
    lib = load_library()
    k, handles, f, dp, _, lp, nr, status, keep = _region_batch_inputs(ctxs, depths, labels, n_regions, fmt, None, on_device)
    vp = ctypes.c_void_p
    outs, results = _outs(rows_out, k, "rows_out"), (RegionBoxesResult * k)()
    want, shapes, sp = _second_out(shapes_out, k, "shapes_out", "the shape rows", on_device, _shape_rows, nr)
    if on_device:
        rows = [None] * k
        rp = (vp * k)(*[_opt_ptr(o) for o in outs])
    else:
        rows = [_box_rows(o, nr[i]) for i, o in enumerate(outs)]
        rp = (vp * k)(*[vp(r.ctypes.data) if len(r) else None for r in rows])
    where = 1 if on_device else 0
    rc = lib.f3ds_region_boxes_batch(handles, k, ctypes.byref(f), dp, lp, nr, float(plane_tol), where, rp, sp, where, results, status.ctypes.data)
    _batch_done(lib, rc, status)
    ok = status == 0
    if want:
        return [(rows[i] if ok[i] else None, shapes[i] if ok[i] else None, results[i] if ok[i] else None) for i in range(k)], status
    return [(rows[i] if ok[i] else None, results[i] if ok[i] else None) for i in range(k)], status


def cloud_regions_batch(ctxs, points, labels, n_regions, params=None, rows_out=None, boxes_out=None, counts=None, on_device=False):
    """f3ds_cloud_regions_batch: Context.cloud_regions for every frame at once; every frame has its own point count (0 is legal).  points / labels: lists of
    arrays (a points entry may be None: the context's own records), or of device pointers / torch tensors with ``on_device`` (``counts`` then gives the point
    counts, ``rows_out`` / ``boxes_out`` are lists of device buffers).  ``boxes_out``: None, ``True`` (host form: new arrays) or a list of buffers, for every
    frame or for none.  Returns ([(rows, CloudRegionsResult)], status), or ([(rows, boxes, CloudRegionsResult)], status) with boxes."""
    lib = load_library()
    k = len(ctxs)
    if k < 1:
        raise ValueError("a batch needs at least one context")
    for name, seq in (("points", points), ("labels", labels), ("n_regions", n_regions)):
        if len(seq) != k:
            raise ValueError("%s must hold one entry per context" % name)
    vp = ctypes.c_void_p
    handles = (vp * k)(*[c.handle for c in ctxs])
    nr = (ctypes.c_uint32 * k)(*[int(x) for x in n_regions])
    status = np.full(k, _STATUS_UNSET, np.int32)
    outs, results = _outs(rows_out, k, "rows_out"), (CloudRegionsResult * k)()
    spare = np.zeros(24, np.float32)      # (an empty cloud, and the boxes of a frame without regions, still have an address)
    want, boxes, bp = _second_out(boxes_out, k, "boxes_out", "the boxes", on_device, _box_rows, nr, spare)
    if on_device:
        if counts is None or len(counts) != k:
            raise ValueError("on_device needs the point counts")
        keep, cnt = None, (ctypes.c_size_t * k)(*[int(x) for x in counts])
        pp = (vp * k)(*[_opt_ptr(x) for x in points]); lp = (vp * k)(*[_device_ptr(x) for x in labels])
        rows = [None] * k
        rp = (vp * k)(*[_opt_ptr(o) for o in outs])
    else:
        keep = [_cloud_inputs(p, lab) for p, lab in zip(points, labels)]
        cnt = (ctypes.c_size_t * k)(*[len(x[1]) for x in keep])
        pp = (vp * k)(*[None if x[0] is None else vp(_ptr(x[0]) or spare.ctypes.data) for x in keep])
        lp = (vp * k)(*[vp(_ptr(x[1]) or spare.ctypes.data) for x in keep])
        rows = [_cloud_rows(o, nr[i]) for i, o in enumerate(outs)]
        rp = (vp * k)(*[vp(r.ctypes.data) if len(r) else None for r in rows])
    where = 1 if on_device else 0
    rc = lib.f3ds_cloud_regions_batch(handles, k, pp, cnt, lp, nr, ctypes.byref(params) if params is not None else None, where, rp, bp, where, results, status.ctypes.data)
    _batch_done(lib, rc, status)
    ok = status == 0
    if want:
        return [(rows[i] if ok[i] else None, boxes[i] if ok[i] else None, results[i] if ok[i] else None) for i in range(k)], status
    return [(rows[i] if ok[i] else None, results[i] if ok[i] else None) for i in range(k)], status


def _capped_call(fn, results, status, batch, param, on_device, before=(), after=()):
    """call(rows pointer array or None, caps, n_out, frames[, status]) -> rc of a batch function whose row counts the device decides: it runs the listed frames
    of ``batch`` = (handles, format, depth pointers, label pointers, region counts) through fn(handles, m, format, depths, labels, n_regions, param, on_device,
    *before, rows, caps, *after, on_device, n_out, results, status) and keeps the results of the frames it reached.  before / after: per-frame pointer arrays
    (or None) of the whole batch."""
    handles, f, dp, lp, nr = batch
    where = 1 if on_device else 0

    def call(rp, caps, n_out, frames, st=status):
        m = len(frames)
        pick = lambda arr, ty=ctypes.c_void_p: None if arr is None else (ty * m)(*[arr[i] for i in frames])
        sub_res = (results._type_ * m)()
        rc = fn(pick(handles), m, ctypes.byref(f), pick(dp), pick(lp), pick(nr, ctypes.c_uint32), param, where, *[pick(a) for a in before], rp, caps, *[pick(a) for a in after],
                where, n_out, sub_res, st.ctypes.data)
        for j, i in enumerate(frames):
            if st[j] != _STATUS_UNSET:
                results[i] = sub_res[j]
        return rc
    return call


def _capped_rows_batch(call, k, rows_out, on_device, dtype):
    """The rows of the batch calls whose row counts the device decides (contacts, components).  call(rows pointer array or None, caps, n_out, frames) -> rc runs
    the listed frames; host form without ``rows_out[i]``: a buffer that turns out too small is grown from the count and those frames run once more."""
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    outs = _outs(rows_out, k, "rows_out")
    n_out = (sz * k)()
    frames = list(range(k))
    if on_device:
        pairs = [(None, 0) if o is None else (_device_ptr(o[0]), int(o[1])) for o in outs]
        rp = (vp * k)(*[p for p, _ in pairs]) if any(o is not None for o in outs) else None
        rc = call(rp, (sz * k)(*[c for _, c in pairs]), n_out, frames)
        return rc, [None] * k, n_out
    bufs = []
    for o in outs:
        if o is not None and not (isinstance(o, np.ndarray) and o.dtype == dtype and o.flags.c_contiguous and o.ndim == 1):
            raise ValueError("rows_out[i] must be a contiguous one-dimensional array of the rows' dtype (%d bytes per row)" % dtype.itemsize)
        bufs.append(np.empty(_CONTACT_ROWS_FIRST, dtype) if o is None else o)
    rp = (vp * k)(*[vp(b.ctypes.data) if len(b) else None for b in bufs])
    rc = call(rp, (sz * k)(*[len(b) for b in bufs]), n_out, frames)
    return rc, bufs, n_out


def _capped_deliver(lib, call, rc, status, bufs, n_out, rows_out, dtype, on_device):
    """after the first run: the frames without a buffer of the caller's that were one short run again with room for all; then the rows of the frames that are OK"""
    _batch_done(lib, rc, status)
    k = len(status)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    outs = _outs(rows_out, k, "rows_out")
    if not on_device:
        again = [i for i in range(k) if status[i] == ERR_CAPACITY and outs[i] is None]
        if again:
            for i in again:
                bufs[i] = np.empty(n_out[i], dtype)
            sub = np.full(len(again), _STATUS_UNSET, np.int32)
            sub_n = (sz * len(again))()
            rc = call((vp * len(again))(*[vp(bufs[i].ctypes.data) for i in again]), (sz * len(again))(*[len(bufs[i]) for i in again]), sub_n, again, sub)
            _batch_done(lib, rc, sub)
            for j, i in enumerate(again):
                status[i] = sub[j]; n_out[i] = sub_n[j]
        return [(bufs[i][:n_out[i]] if outs[i] is not None else bufs[i][:n_out[i]].copy()) if status[i] == 0 else None for i in range(k)]
    return [None] * k


def region_contacts_batch(ctxs, depths, labels, n_regions, fmt, depth_tol=0.05, rows_out=None, on_device=False):
    """f3ds_region_contacts_batch: Context.region_contacts for every frame at once (lists as in region_table_batch; ``rows_out``: a list of arrays to fill, or with
    ``on_device`` of ``(device pointer, capacity in rows)`` / None).  Returns ([(rows, RegionContactsResult)], status)."""
    lib = load_library()
    k, handles, f, dp, _, lp, nr, status, keep = _region_batch_inputs(ctxs, depths, labels, n_regions, fmt, None, on_device)
    results = (RegionContactsResult * k)()
    call = _capped_call(lib.f3ds_region_contacts_batch, results, status, (handles, f, dp, lp, nr), float(depth_tol), on_device)
    rc, bufs, n_out = _capped_rows_batch(call, k, rows_out, on_device, REGION_CONTACT_DTYPE)
    rows = _capped_deliver(lib, call, rc, status, bufs, n_out, rows_out, REGION_CONTACT_DTYPE, on_device)
    return [(rows[i], results[i] if status[i] != ERR_ARG else None) for i in range(k)], status


def region_joints_batch(ctxs, depths, labels, n_regions, fmt, params=None, rows_out=None, shapes_out=None, on_device=False):
    """f3ds_region_joints_batch: Context.region_joints for every frame at once (lists as in region_contacts_batch).  ``shapes_out``: None, ``True`` (host form: new
    arrays) or a list of buffers, for every frame or for none.  Returns ([(rows, RegionJointsResult)], status), or ([(rows, shapes, RegionJointsResult)], status)
    with shapes."""
    lib = load_library()
    k, handles, f, dp, _, lp, nr, status, keep = _region_batch_inputs(ctxs, depths, labels, n_regions, fmt, None, on_device)
    results = (RegionJointsResult * k)()
    want, shapes, sp = _second_out(shapes_out, k, "shapes_out", "the shape rows", on_device, _shape_rows, nr)
    call = _capped_call(lib.f3ds_region_joints_batch, results, status, (handles, f, dp, lp, nr), ctypes.byref(params) if params is not None else None, on_device, after=(sp,))
    rc, bufs, n_out = _capped_rows_batch(call, k, rows_out, on_device, REGION_JOINT_DTYPE)
    rows = _capped_deliver(lib, call, rc, status, bufs, n_out, rows_out, REGION_JOINT_DTYPE, on_device)
    ok = [status[i] != ERR_ARG for i in range(k)]
    if want:
        return [(rows[i], shapes[i] if ok[i] else None, results[i] if ok[i] else None) for i in range(k)], status
    return [(rows[i], results[i] if ok[i] else None) for i in range(k)], status


def region_components_batch(ctxs, depths, labels, n_regions, fmt, depth_tol=0.05, min_pixels=1, rows_out=None, comp_out=None, on_device=False):
    """f3ds_region_components_batch: Context.region_components for every frame at once (lists as in region_contacts_batch; ``comp_out``: with ``on_device`` a list
    of device buffers of width * height words).  Returns ([(comp_labels, rows, RegionComponentsResult)], status)."""
    lib = load_library()
    k, handles, f, dp, _, lp, nr, status, keep = _region_batch_inputs(ctxs, depths, labels, n_regions, fmt, None, on_device)
    vp = ctypes.c_void_p
    prm, results = ComponentParams(float(depth_tol), int(min_pixels)), (RegionComponentsResult * k)()
    if on_device:
        if comp_out is None or len(comp_out) != k:
            raise ValueError("on_device needs one device image per context in comp_out")
        comps = [None] * k
        kp = (vp * k)(*[_opt_ptr(o) for o in comp_out])
    else:
        comps = [np.empty((int(fmt.height), int(fmt.width)), np.uint32) for _ in range(k)]
        kp = (vp * k)(*[vp(c.ctypes.data) for c in comps])
    call = _capped_call(lib.f3ds_region_components_batch, results, status, (handles, f, dp, lp, nr), ctypes.byref(prm), on_device, before=(kp,))
    rc, bufs, n_out = _capped_rows_batch(call, k, rows_out, on_device, REGION_COMPONENT_DTYPE)
    rows = _capped_deliver(lib, call, rc, status, bufs, n_out, rows_out, REGION_COMPONENT_DTYPE, on_device)
    return [(comps[i] if status[i] != ERR_ARG else None, rows[i], results[i] if status[i] != ERR_ARG else None) for i in range(k)], status


def best_level(thresholds, scores):
    """f3ds_best_level: Clustering::best_thresh over scored levels: the index of the best level by F-score (levels by ascending
    threshold, the first strictly greater F-score wins), or -1 when no level has fscore > 0.  ``scores``: Performance records."""
    lib = load_library()
    t = np.ascontiguousarray(np.atleast_1d(np.asarray(thresholds, np.float32)).ravel())
    k = len(t)
    if len(scores) != k:
        raise ValueError("one score record per threshold is required")
    ps = (Performance * max(k, 1))(*scores)
    best = ctypes.c_int(-2)
    _check(lib, lib.f3ds_best_level(t.ctypes.data, ps, k, ctypes.byref(best)))
    return best.value


def segment(points, params=None, device=0):
    """XYZRGBA frame -> (per-point region ids, Result).  One-shot convenience wrapper."""
    ctx = Context(device)
    try:
        labels = ctx.segment(points, params or launch_params())
        res = Result()
        ctypes.memmove(ctypes.byref(res), ctypes.byref(ctx.result), ctypes.sizeof(Result))
        return labels, res
    finally:
        ctx.close()


# ---- mirror of the reference's classes -------------------------------------------------------------
class SupervoxelClustering:
    """The nine-call VCCS sequence of main() (supervoxel_clustering.cpp:348-367) as one object."""

    def __init__(self, voxel_resolution, seed_resolution, context=None):
        self.ctx = context or Context()
        self.params = default_params(voxel_res=voxel_resolution, seed_res=seed_resolution)
        self.cloud = None

    def setUseSingleCameraTransform(self, val):
        self.params.use_transform = 1 if val else 0

    def setInputCloud(self, points):
        self.cloud = np.ascontiguousarray(points, np.float32).reshape(-1, 4)

    def setColorImportance(self, v):
        self.params.w_color = v

    def setSpatialImportance(self, v):
        self.params.w_spatial = v

    def setNormalImportance(self, v):
        self.params.w_normal = v

    def extract(self):
        """extract(supervoxel_clusters) (:356): runs the frame and returns the supervoxels (see Context.supervoxels)."""
        if self.cloud is None:
            raise LogicError(-5, "setInputCloud first")
        self.ctx.segment(self.cloud, self.params)
        self._extracted = True
        return self.ctx.supervoxels()

    def getVoxelCentroidCloud(self):               # :359 -> (xyz, rgba)
        xyz, rgba, _ = self.ctx.voxel_centroid_cloud()
        return xyz, rgba

    def getLabeledVoxelCloud(self):                # voxel centroids with their supervoxel label
        xyz, _, lab = self.ctx.voxel_centroid_cloud()
        return xyz, lab

    def makeSupervoxelNormalCloud(self):           # :360 -> (centroid xyz, normal) per supervoxel
        sv = self.ctx.supervoxels()
        return sv["xyz"], sv["normal"]

    def refineSupervoxels(self, num_itr):          # :371 -> refined per-voxel labels / normals and supervoxel map
        return self.ctx.refine_supervoxels(num_itr)

    def getSupervoxelAdjacency(self):              # :365
        return self.ctx.supervoxel_adjacency()


class Clustering:
    """Mirror of ``class Clustering`` (clustering.h:84-212) on top of the device path."""

    def __init__(self, c=LAB_CIEDE00, g=NORMALS_DIFF, m=ADAPTIVE_LAMBDA):
        self.delta_c_type, self.delta_g_type = c, g
        self.set_merging(m)
        self._super = None
        self._labels = None

    def set_delta_c(self, d):
        self.delta_c_type = d

    def set_delta_g(self, d):
        self.delta_g_type = d

    def set_merging(self, m):                      # clustering.cpp:562-567
        self.merging_type, self.lambda_, self.bins_num = m, 0.5, 500

    def set_lambda(self, l):                       # clustering.cpp:574-582
        if self.merging_type != MANUAL_LAMBDA:
            raise LogicError(-5, "Lambda can be set only if the merging criterion is set to MANUAL_LAMBDA")
        if l < 0 or l > 1:
            raise ValueError("Argument outside range [0, 1]")
        self.lambda_ = l

    def set_bins_num(self, b):                     # clustering.cpp:589-597
        if self.merging_type != EQUALIZATION:
            raise LogicError(-5, "Bins number can be set only if the merging criterion is set to EQUALIZATION")
        if b < 0:
            raise ValueError("Argument lower than 0")
        self.bins_num = b

    def get_delta_c(self):
        return self.delta_c_type

    def get_delta_g(self):
        return self.delta_g_type

    def get_merging(self):
        return self.merging_type

    def get_lambda(self):
        return self.lambda_

    def get_bins_num(self):
        return self.bins_num

    def set_initialstate(self, segm, adj=None, context=None):
        """set_initialstate(segm, adj) (clustering.cpp:605-612).  Two forms:
        * ``segm`` = {label: dict(voxels_xyz, voxels_rgba, centroid, normal)}, ``adj`` = iterable of (first, second) in multimap
          iteration order -- supervoxels of ANY algorithm, as the reference's signature takes them (f3ds_cluster_supervoxels);
        * ``segm`` = a SupervoxelClustering object, ``adj`` omitted -- its extract() result is already device-resident."""
        if adj is None and isinstance(segm, SupervoxelClustering):
            self._super, self._user = segm, None
            self._segmented = False
            return
        if adj is None:
            raise TypeError("set_initialstate(segm, adj): the adjacency map is missing")
        self._user = (pack_supervoxels(segm), np.array(list(adj), np.uint32).reshape(-1, 2), context or Context())
        self._super = _UserState(self._user[2])
        self._segmented = False

    def _params(self, threshold):
        p = self._super.params.copy()
        p.color_metric, p.geom_metric, p.merging = self.delta_c_type, self.delta_g_type, self.merging_type
        p.lambda_ = self.lambda_ if self.merging_type == MANUAL_LAMBDA else 0.0
        p.bins = self.bins_num if self.merging_type == EQUALIZATION else 0
        p.threshold = threshold
        return p

    def cluster(self, threshold):                  # clustering.cpp:670-679
        if self._super is None:
            raise LogicError(-5, "Cannot call 'cluster' before setting an initial state with 'set_initialstate'")
        ctx = self._super.ctx
        if not self._segmented and getattr(self, "_user", None):
            self._region_of_sv, self._labels = ctx.cluster_supervoxels(self._user[0], self._user[1], self._params(threshold))
            self._segmented = True
        elif not self._segmented:
            self._labels = ctx.segment(self._super.cloud, self._params(threshold))
            self._segmented = True
        else:
            self._labels = ctx.recluster(self._params(threshold))
            if getattr(self, "_user", None):
                # a later cluster(t) moves the supervoxels to other regions: F3DS_DBG_SV_REGION lists the surviving label per supervoxel in ascending
                # label order, the caller's rows may be in any order
                lab = np.asarray(self._user[0]["label"], np.uint32)
                reg = ctx.debug("SV_REGION")
                out = np.zeros(len(lab), np.uint32)
                out[np.argsort(lab, kind="stable")] = reg
                self._region_of_sv = out
        if self.merging_type == ADAPTIVE_LAMBDA:
            self.lambda_ = ctx.result.lambda_

    def all_thresh(self, truth_point_labels, start_thresh, end_thresh, step_thresh):      # clustering.cpp:691-741
        """{threshold: performanceSet dict} over the sweep.  As in the reference the state is left clustered at the LAST threshold of the
        sweep (:718-726); IndexError (std::out_of_range, :694-698) for bounds outside [0, 1]; start > end are swapped (:699-705)."""
        if self._super is None:
            raise LogicError(-5, "Cannot call 'all_thresh' before setting an initial state with 'set_initialstate'")
        if getattr(self, "_user", None):
            raise LogicError(-5, "all_thresh needs the frame's points (ground truth is per input point): use a SupervoxelClustering state")
        if start_thresh < 0 or start_thresh > 1 or end_thresh < 0 or end_thresh > 1 or step_thresh < 0 or step_thresh > 1:
            raise IndexError("start_thresh, end_thresh and/or step_thresh outside of range [0, 1]")
        ctx = self._super.ctx
        if not self._segmented:
            ctx.segment(self._super.cloud, self._params(min(start_thresh, end_thresh)))
            self._segmented = True
        bt, bp, table, self._labels = ctx.auto_threshold(self._params(0.0), truth_point_labels, start_thresh, end_thresh, step_thresh)
        if table:
            self._labels = ctx.recluster(self._params(max(table)))      # (f3ds_auto_threshold leaves the context at the best threshold: main()'s use)
        if self.merging_type == ADAPTIVE_LAMBDA:
            self.lambda_ = ctx.result.lambda_
        return table

    @staticmethod
    def best_thresh(all_performances):             # clustering.cpp:748-774: first strictly greater F-score, (0, zeros) if none
        best_t, best_p = 0.0, {k: 0.0 for k in ("voi", "precision", "recall", "fscore", "wov", "fpr", "fnr")}
        for t in sorted(all_performances):
            if all_performances[t]["fscore"] > best_p["fscore"]:
                best_t, best_p = t, all_performances[t]
        return best_t, best_p

    def eval_performance(self, truth_point_labels):
        """Testing(get_labeled_cloud(), truth_cloud).eval_performance() (src/supervoxel_clustering.cpp:462-463)."""
        return self._super.ctx.evaluate(truth_point_labels).as_dict()

    def get_labeled_cloud(self):                   # clustering.cpp:640-663 -> (xyz, label)
        xyz, lab, _ = self._super.ctx.voxel_cloud()
        return xyz, lab

    def get_colored_cloud(self):                   # clustering.cpp:631-633 -> (xyz, rgba)
        xyz, _, rgba = self._super.ctx.voxel_cloud()
        return xyz, rgba

    @staticmethod
    def label2color(xyz, labels):                  # clustering.cpp:793-812 -> (xyz, rgba): the lookup-table colour of every label, opaque alpha
        labels = np.asarray(labels, np.uint32)
        table = np.array([label_color(i) for i in range(256)], np.uint32)
        return np.asarray(xyz, np.float32), (table[labels % 256] | np.uint32(0xFF000000)).astype(np.uint32)

    @staticmethod
    def color2label(xyz, rgba):                    # clustering.cpp:824-846 -> (xyz, label): one label per distinct colour, numbered in order of first appearance
        rgba = np.asarray(rgba, np.uint32)
        uniq, first, inv = np.unique(rgba, return_index=True, return_inverse=True)
        rank = np.empty(len(uniq), np.uint32)
        rank[np.argsort(first, kind="stable")] = np.arange(len(uniq), dtype=np.uint32)
        return np.asarray(xyz, np.float32), rank[inv].astype(np.uint32)

    def get_region_of_supervoxel(self):
        """After set_initialstate(segm, adj) + cluster(t): label of the region every input supervoxel ended in at the LAST threshold, in the row
        order of the supervoxel arrays."""
        return getattr(self, "_region_of_sv", None)

    def get_point_labels(self):
        """Per input point region id (the composition with pcl getLabeledCloud); per input VOXEL after
        set_initialstate(segm, adj)."""
        return self._labels

    def get_currentstate(self):                    # clustering.cpp:619-624
        """(segments, adjacency): segments = {label: dict(voxels_xyz, voxels_rgba, voxel_index, centroid, normal, mean_rgb)} of the merged
        regions (state.segments), adjacency = (K, 2) array of label pairs a < b (weight2adj(state.weight_map))."""
        ctx = self._super.ctx
        r = ctx.regions()
        xyz, rgba, idx = ctx.region_voxels()
        segm, o = {}, 0
        for k in range(len(r["label"])):
            n = int(r["n_voxels"][k])
            segm[int(r["label"][k])] = dict(voxels_xyz=xyz[o:o + n], voxels_rgba=rgba[o:o + n], voxel_index=idx[o:o + n], centroid=r["xyz"][k],
                                            normal=r["normal"][k], mean_rgb=r["rgb"][k])
            o += n
        return segm, ctx.region_adjacency()


class _UserState:
    """What Clustering keeps in place of a SupervoxelClustering object after set_initialstate(segm, adj)."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.params = default_params()
        self.cloud = None
