"""What the narrow-launch tests run, and why that is enough (shared by test_narrow_launch_cpu.py and test_narrow_launch_gpu.py).

Every wide kernel of csrc/f3ds_kernels.inc is a grid-stride loop: a workgroup takes `items` consecutive elements per trip and comes back
`width * wgs_per_width` workgroups further on.  At its default width (2048 workgroups for a lone frame, 192 in a batch of 16) a golden frame is
done in one trip, so nothing a second trip needs -- LDS tiles staged again, wave-wide operations with lanes that have left, a remainder in the last
trip -- is ever run.  The development switch F3DS_GRID_CAP=<width> caps every launch at `width` workgroups per frame; FAMILIES lists the loops by what
they stride over, and `run_covers()` says whether a frame of given sizes makes such a loop go round at least three times and end on a ragged trip.

The table is read off the kernels, not off the launches: `items` is what ONE workgroup does in ONE trip.
  * d_bbox is launched n / 2048 wide but strides by 256 points like every other point loop (eight trips at any width): it sits with them.
  * d_neighbors keeps the 27 x 64 results of 64 voxels in LDS per trip (launched 27 V / 256 wide: one trip until the cap bites).
  * d_centroid is launched S0 / 4 wide (a wave per helper), but a lane asks for a group of four helpers, so a workgroup looks at 256 helpers per trip.
  * d_sweep_claim and d_sweep_R_round ask marked_pairs() about 64 tile pairs at once, one per lane: their OUTER loops stride 64 * 256 voxels per
    workgroup, the inner ones one tile pair of 256.
  * stage 0's tile path (d_tile_keys, d_tile_place) runs 16 workgroups per unit of width, one 4096-point tile each per trip.
"""
import collections
import json
import os

from conftest import ROOT

Family = collections.namedtuple("Family", "name size items wgs_per_width kernels only", defaults=(None,))      # only: the cases whose parameters run these kernels at all

FAMILIES = [
    Family("points/256", "n", 256, 1, "d_bbox d_keys d_heads d_segstart d_point_gather d_point_labels d_truth_accum d_level_points d_evl_heads d_evl_reduce d_evl_col_keys"),
    Family("tiles/1", "tiles", 1, 16, "d_tile_keys d_tile_place"),
    Family("V/256", "V", 256, 1, "d_sweep_R_pre d_sweep_R d_sweep_R_round d_sweep_claim (tile pairs) d_edges d_seed_keys d_refine_normals d_contingency d_truth_color "
                                  "d_voxel_gather_accum d_voxel_accum d_voxel_list_accum d_evl_base_keys"),
    Family("V/16384", "V", 64 * 256, 1, "d_sweep_R_round d_sweep_claim (outer loop: 64 tile pairs per marked_pairs() word)"),
    Family("V/4096", "V", 4096, 1, "d_vox_table"),
    Family("V/64", "V", 64, 1, "d_neighbors"),
    Family("C/256", "C", 256, 1, "d_cell_hash d_seed_compact"),
    Family("E/256", "E", 256, 1, "d_iota d_edge_init d_edge_deltas d_edge_weights"),
    Family("2E/256", "2E", 256, 1, "d_cdf_hist", ("rgbd_160x120_equalization",)),      # (merging = EQUALIZATION)
    Family("S0/256", "S0", 256, 1, "d_helper_own d_helper_init d_reseed_own d_reseed_init d_region_reset d_edges_ghost d_contingency_ghost d_refine_ghost_L d_evl_ghosts "
                                   "d_centroid (64 groups of four helpers per trip)"),
]

WIDTHS = (1, 3, 8)
STAGE0 = ("sort", "tiles")

# (case of golden_cases.GOLDEN_CASES, widths it runs at).  Every case runs with stage 0 on either path.
SINGLE_CASES = [
    ("rgbd_160x120", WIDTHS),
    ("rgbd_160x120_desc_leaf_order", WIDTHS),
    ("rgbd_160x120_no_transform", WIDTHS),                # depth 8: the two-word voxel table
    ("rgbd_160x120_equalization", WIDTHS),                # the 2 E histogram
    ("rgbd_320x240_ghosts", WIDTHS),                      # ghost paths
    ("rgbd_320x240_large_supervoxels", WIDTHS),           # a wave per helper, window scan, 56 sweeps
    # 781.25 blocks of points; at width 1 the only frame whose 127 k voxels send the sweeps' outer loops round (7.8 trips) and whose 49 point tiles take 16 workgroups 3.1 trips
    ("fused_200k_nan_lambda", (1, 8)),
]

# frames stage 0's tile path hands back to the sort path (a tile of 4096 points may hold 1280 distinct voxels): 0.8 voxels per point; an unorganised cloud
TILE_PATH_REFUSES = ("rgbd_160x120_no_transform", "fused_200k_nan_lambda")

SWEEP_VARIANT_WIDTH = 3
SWEEP_VARIANTS = [
    dict(F3DS_INC_SHIFT="-1"),
    dict(F3DS_INC_SHIFT="32"),
    dict(F3DS_SWEEP_TILES="0"),
    dict(F3DS_SWEEP_TILE_HOLES="3"),
    dict(F3DS_INC_SHIFT="32", F3DS_R_ROUNDS_RUN="1"),     # every incremental sweep falls back to d_sweep_R's whole-grid loop
]
SWEEP_VARIANT_CASES = ["rgbd_320x240_ghosts", "rgbd_320x240_large_supervoxels"]
SWEEP_VARIANT_ARRAYS = ("VOXEL_SVLABEL", "VOXEL_DIST", "SV_CENTROID", "MERGES")

ENTRY_WIDTHS = (1, 3)
ENTRY_CASES = ["rgbd_160x120", "rgbd_320x240_ghosts"]

BATCH_SIZES = (9, 17)                                     # one and two full groups of eight frames (f3ds_vblock) plus a remainder
BATCH_WIDTHS = (1, 3)

LEVEL_WIDTHS = (1, 3)
LEVEL_CASES = ["rgbd_160x120", "rgbd_160x120_equalization", "rgbd_320x240_ghosts"]


def golden_sizes(name):
    """The loop bounds of a golden case, from the summary committed in tests/golden/oracle_golden.json."""
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_golden.json")))[name]["summary"]
    n = int(s["n_points"])
    return {"n": n, "tiles": (n + 4095) // 4096, "V": int(s["n_voxels"]), "C": int(s["n_seed_cells"]), "E": int(s["n_edges"]), "2E": 2 * int(s["n_edges"]), "S0": int(s["n_seeds"])}


def trips(work, items, workgroups):
    """(trips of the busiest workgroup, whether the last trip is ragged) of a grid-stride loop over `work` elements, `items` per workgroup and trip.
    Ragged: some but not all workgroups have work in it, or one of them is only partly filled."""
    chunks = -(-work // items)
    t = -(-chunks // workgroups)
    ragged = chunks % workgroups != 0 or work % items != 0
    return t, ragged


def run_covers(family, sizes, width):
    t, ragged = trips(sizes[family.size], family.items, width * family.wgs_per_width)
    return t >= 3 and ragged
