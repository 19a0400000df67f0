"""The batch forms of the five region calls without a device: the five symbols and the package's functions exist, the calls refuse what needs no device to
refuse (NULL ctxs, nctx < 1, a NULL context entry) and leave `status` alone then, the package's functions validate their lists, and li_stage_layout -- the staging
layout of a batch, a pure function of the frames' byte counts (csrc/f3ds_label_image.h) -- is restated here and checked on the batches of the GPU test."""
import ctypes
import types

import numpy as np
import pytest

import region_batch_common as C

UNSET = C.UNSET
HEAD = 32      # LI_HEAD_BYTES


def test_symbols_and_functions_exist(P):
    lib = P.load_library()
    for call in C.CALLS:
        assert hasattr(lib, "f3ds_region_%s_batch" % call) and callable(getattr(P, "region_%s_batch" % call))


@pytest.mark.parametrize("call", C.CALLS)
def test_refusals_that_need_no_device(P, call):
    B = C.batch(P, "tiny32")
    assert C.run(P, [], B, call, "host", handles=ctypes.POINTER(ctypes.c_void_p)())["rc"] == P.ERR_ARG      # NULL ctxs
    vp = ctypes.c_void_p
    for handles in ((vp * 3)(None, None, None), (vp * 3)(None, vp(8), vp(16))):      # (a NULL entry is found before any context is looked into)
        out = C.run(P, [], B, call, "host", handles=handles)
        assert out["rc"] == P.ERR_ARG and (out["status"] == UNSET).all() and all(C.untouched(P, call, fr) for fr in out["frames"])
    assert C.run(P, [], B, call, "host", handles=(vp * 3)(None, None, None), status=False)["rc"] == P.ERR_ARG      # status may be NULL


def test_the_package_validates_its_lists(P):
    B = C.batch(P, "tiny32")
    fake = [types.SimpleNamespace(handle=ctypes.c_void_p(0)) for _ in range(3)]
    d, l, k = [f["depth"] for f in B.frames], [f["labels"] for f in B.frames], [f["K"] for f in B.frames]
    for call in C.CALLS:
        fn = getattr(P, "region_%s_batch" % call)
        with pytest.raises(ValueError):
            fn([], [], [], [], B.fmt)
        with pytest.raises(ValueError):
            fn(fake, d[:2], l, k, B.fmt)
        with pytest.raises(ValueError):
            fn(fake, d, l[:1], k, B.fmt)
        with pytest.raises(ValueError):
            fn(fake, d, l, k + [1], B.fmt)
        with pytest.raises(ValueError):
            fn(fake, d, l, k, B.fmt, rows_out=[None])
        with pytest.raises(P.F3dsError):      # NULL contexts: the library refuses the call as a whole, and that is raised
            fn(fake, d, l, k, B.fmt)
    color = C.color_of(B, 0, "rgb8")
    with pytest.raises(ValueError):
        P.region_table_batch(fake, d, l, k, B.fmt, colors=[color, None, color])      # mixed: one command sequence for the batch
    with pytest.raises(ValueError):
        P.region_table_batch(fake, d, l, k, B.fmt, colors=[color])
    with pytest.raises(ValueError):
        P.region_boxes_batch(fake, d, l, k, B.fmt, shapes_out=[np.zeros(k[0], P.REGION_SHAPE_DTYPE), None, None])
    with pytest.raises(P.F3dsError):
        P.region_table_batch(fake, d, l, k, B.fmt, colors=[None, None, None])      # (no colour for any frame is no colour)


# ---- the staging layout ----------------------------------------------------------------------------------------------------------------------------------------
def stage_layout(fixed, stage_rows, row_bytes, first_rows):
    """li_stage_layout restated: ([(at, rows_at, first)], first_bytes, total)"""
    a8 = lambda x: (x + 7) & ~7
    n = len(fixed)
    off = n * HEAD
    slot = []
    for i in range(n):
        at = off; off += a8(fixed[i])
        short = stage_rows is not None and stage_rows[i] <= first_rows
        slot.append([at, off, stage_rows[i] if short else 0])
        if short:
            off += a8(stage_rows[i] * row_bytes)
    first_bytes, first_long = off, True
    for i in range(n):
        if stage_rows is None or stage_rows[i] <= first_rows:
            continue
        slot[i][1] = off
        if first_long:
            slot[i][2], first_bytes, first_long = first_rows, off + first_rows * row_bytes, False
        off += a8(stage_rows[i] * row_bytes)
    return slot, first_bytes, off


def test_the_staging_layout_keeps_the_frames_apart(P):
    """heads first and contiguous, payloads 8-byte aligned and disjoint, everything the first download promises inside it; one frame is the lone call's layout"""
    rng = np.random.default_rng(5)
    for trial in range(200):
        n = int(rng.integers(1, 9))
        fixed = [int(x) for x in rng.choice([0, 4, 12, 72, 84 * 23, 4 * 5917], n)]
        rows = None if trial % 3 == 0 else [int(x) for x in rng.choice([0, 1, 64, 2048, 2049, 11834], n)]
        rb = int(rng.choice([12, 40]))
        slot, first_bytes, total = stage_layout(fixed, rows, rb, 2048)
        spans = [(0, n * HEAD)]
        for i, (at, rows_at, first) in enumerate(slot):
            assert at % 8 == 0 and rows_at % 8 == 0 and at >= n * HEAD
            spans.append((at, at + fixed[i]))
            assert at + fixed[i] <= first_bytes
            if rows is not None:
                spans.append((rows_at, rows_at + rows[i] * rb))
                assert first == min(rows[i], 2048) if rows[i] <= 2048 else first in (0, 2048)
                assert first == 0 or rows_at + first * rb <= first_bytes      # (nothing is promised of a long array that is not the first)
        spans = sorted(s for s in spans if s[1] > s[0])
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= total and first_bytes <= total
        if rows is not None:
            assert sum(1 for i, s in enumerate(slot) if rows[i] > 2048 and s[2]) == min(1, sum(1 for r in rows if r > 2048))
    # one frame: the head, the image, the rows right behind it, the first 2048 of them in the first download
    slot, first_bytes, total = stage_layout([4 * 5917], [5000], 12, 2048)
    assert slot == [[HEAD, HEAD + 4 * 5917 + 4, 2048]] and first_bytes == slot[0][1] + 2048 * 12 and total == slot[0][1] + 5000 * 12


def test_the_layout_in_the_header_is_the_one_restated(P):
    """li_stage_layout computes what stage_layout() above says, on the batches of the test before this one and at the rows either side of the first download"""
    rng = np.random.default_rng(5)
    cases = [([4 * 5917], [5000], 12, 2048), ([0], None, 12, 2048), ([4, 12], [2048, 2049], 40, 2048), ([72, 0, 4], [2049, 2049, 0], 12, 2048)]
    for trial in range(200):
        n = int(rng.integers(1, 9))
        fixed = [int(x) for x in rng.choice([0, 4, 12, 72, 84 * 23, 4 * 5917], n)]
        rows = None if trial % 3 == 0 else [int(x) for x in rng.choice([0, 1, 64, 2048, 2049, 11834], n)]
        cases.append((fixed, rows, int(rng.choice([12, 40])), 2048))
    for fixed, rows, rb, first_rows in cases:
        assert P.policy_stage_layout(fixed, rows, rb, first_rows) == stage_layout(fixed, rows, rb, first_rows), (fixed, rows, rb)
