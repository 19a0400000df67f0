"""The label-image calls share their staging on a context (csrc/f3ds_hip.hip, "the label-image frame": one upload trio, one device-side out buffer, one
pinned download buffer for f3ds_region_table, f3ds_region_shapes, f3ds_region_boxes, f3ds_region_contacts and f3ds_region_components; the tracker's private context has the
same upload trio).  So the calls are run here INTERLEAVED on one context and one tracker: two frame sizes in turn (97 x 61 and 33 x 17: the small call runs in
buffers the large one grew, and the reverse), host inputs and rows in turn with device inputs and rows, the table with and without colour, one call in the
middle that fails on a label >= n_regions.  Every result equals the Python references bit for bit, and rows a caller holds on the device from an earlier call
are unchanged after all the later ones.  Once at the default launch width and once at F3DS_GRID_CAP = 1."""
import numpy as np
import pytest

import region_boxes_common as B
import region_components_common as C
import region_contacts_common as CT
import region_shapes_common as S
import region_table_common as R
import track_common as T

pytestmark = pytest.mark.gpu
PREFILL = 0x5A5A5A5A
TOL = 0.05
_refs = {}


def frame(P, name):
    """the two frames and their references, computed once and left unchanged"""
    if name not in _refs:
        w, h, kind, color_kind = dict(big=(97, 61, "u16", "rgba8"), small=(33, 17, "f32", "rgb8"))[name]
        sc = R.scene(P, 1, w, h, kind)
        fmt, depth, lab, K = R.with_color(P, sc["fmt"], color_kind), sc["depth"], sc["labels"], sc["n_regions"]
        color = R.make_color(w, h, color_kind)
        f = dict(fmt=fmt, depth=depth, labels=lab, K=K, color=color, n=w * h,
                 table=R.ref_table(P, fmt, depth, lab, K), table_color=R.ref_table(P, fmt, depth, lab, K, color), shapes=S.ref_shapes(P, fmt, depth, lab, K)[:3],
                 contacts=CT.ref_contacts(P, fmt, depth, lab, K, TOL), components=C.ref_components(P, fmt, depth, lab, K, TOL, 1), boxes=B.ref_boxes(P, fmt, depth, lab, K))
        assert all(f[k][0] == 0 for k in ("table", "table_color", "shapes", "contacts", "components", "boxes")) and len(f["contacts"][1]) > 0
        _refs[name] = f
    return _refs[name]


class Device:
    """a frame's inputs on the device, and output buffers prefilled with 0x5A5A5A5A words"""

    def __init__(self, f):
        import torch
        self.torch = torch
        self.depth = self.put(f["depth"].view(np.uint8))
        self.labels = self.put(f["labels"].view(np.int32))
        self.color = self.put(f["color"].reshape(-1).view(np.uint8))
        torch.cuda.synchronize()

    def put(self, arr):
        return self.torch.from_numpy(np.ascontiguousarray(arr)).cuda()

    def out(self, words):
        t = self.torch.full((max(int(words), 1),), PREFILL, dtype=self.torch.int32, device="cuda")
        self.torch.cuda.synchronize()
        return t

    def get(self, t, dtype, count):
        self.torch.cuda.synchronize()
        return t.cpu().numpy().view(np.uint32)[:count * dtype.itemsize // 4].copy().view(dtype)


def run_sequence(P):
    big, small = frame(P, "big"), frame(P, "small")
    ctx, trk, ref_trk = P.Context(0), P.Tracker(0), T.RefTracker()
    held = []      # (what, check) of rows left on the device: checked again at the end
    try:
        dev = dict(big=Device(big), small=Device(small))

        def table(f, name, where, with_color):
            want = f["table_color" if with_color else "table"]
            if where == "device":
                d = dev[name]; dr = d.out(18 * f["K"])
                _, res = ctx.region_table(d.depth.data_ptr(), d.labels.data_ptr(), f["K"], f["fmt"], color=d.color.data_ptr() if with_color else None,
                                          rows_out=dr.data_ptr(), on_device=True)
                check = lambda: R.assert_rows_equal(P, d.get(dr, P.REGION_ROW_DTYPE, f["K"]), want[1], "table %s" % name)
                check(); held.append(check)
            else:
                rows, res = ctx.region_table(f["depth"], f["labels"], f["K"], f["fmt"], color=f["color"] if with_color else None)
                R.assert_rows_equal(P, rows, want[1], "table %s" % name)
            assert res.as_dict() == want[2]

        def shapes(f, name, where):
            want = f["shapes"]
            if where == "device":
                d = dev[name]; dr = d.out(21 * f["K"])
                _, res = ctx.region_shapes(d.depth.data_ptr(), d.labels.data_ptr(), f["K"], f["fmt"], rows_out=dr.data_ptr(), on_device=True)
                check = lambda: S.assert_rows_equal(P, d.get(dr, P.REGION_SHAPE_DTYPE, f["K"]), want[1], "shapes %s" % name)
                check(); held.append(check)
            else:
                rows, res = ctx.region_shapes(f["depth"], f["labels"], f["K"], f["fmt"])
                S.assert_rows_equal(P, rows, want[1], "shapes %s" % name)
            assert res.as_dict() == want[2]

        def boxes(f, name, where):      # (the shape rows ride along: the boxes' first pass is the shapes' kernels on the shapes' accumulators)
            want = f["boxes"]
            if where == "device":
                d = dev[name]; dr, ds = d.out(24 * f["K"]), d.out(21 * f["K"])
                _, _, res = ctx.region_boxes(d.depth.data_ptr(), d.labels.data_ptr(), f["K"], f["fmt"], rows_out=dr.data_ptr(), shapes_out=ds.data_ptr(), on_device=True)

                def check():
                    B.assert_rows_equal(P, d.get(dr, P.REGION_BOX_DTYPE, f["K"]), want[1], "boxes %s" % name)
                    S.assert_rows_equal(P, d.get(ds, P.REGION_SHAPE_DTYPE, f["K"]), want[2], "boxes' shapes %s" % name)
                check(); held.append(check)
            else:
                rows, shp, res = ctx.region_boxes(f["depth"], f["labels"], f["K"], f["fmt"], shapes_out=True)
                B.assert_rows_equal(P, rows, want[1], "boxes %s" % name)
                S.assert_rows_equal(P, shp, want[2], "boxes' shapes %s" % name)
            assert res.as_dict() == want[3]

        def contacts(f, name, where):
            want = f["contacts"]
            if where == "device":
                d = dev[name]; cap = len(want[1]) + 3; dr = d.out(8 * cap)
                _, res = ctx.region_contacts(d.depth.data_ptr(), d.labels.data_ptr(), f["K"], f["fmt"], TOL, rows_out=(dr.data_ptr(), cap), on_device=True)

                def check():
                    CT.assert_rows_equal(d.get(dr, P.REGION_CONTACT_DTYPE, len(want[1])), want[1], "contacts %s" % name)
                    assert (d.get(dr, np.dtype(np.uint32), 8 * cap)[8 * len(want[1]):] == PREFILL).all()
                check(); held.append(check)
            else:
                rows, res = ctx.region_contacts(f["depth"], f["labels"], f["K"], f["fmt"], TOL)
                CT.assert_rows_equal(rows, want[1], "contacts %s" % name)
            assert res.as_dict() == want[2]

        def components(f, name, where):
            want = f["components"]
            if where == "device":
                d = dev[name]; cap = len(want[2]) + 3; dc, dr = d.out(f["n"]), d.out(3 * cap)
                _, _, res = ctx.region_components(d.depth.data_ptr(), d.labels.data_ptr(), f["K"], f["fmt"], TOL, 1, rows_out=(dr.data_ptr(), cap), comp_out=dc.data_ptr(),
                                                  on_device=True)
                check = lambda: C.assert_same(d.get(dc, np.dtype(np.uint32), f["n"]), d.get(dr, P.REGION_COMPONENT_DTYPE, len(want[2])), want[1], want[2],
                                              "components %s" % name)
                check(); held.append(check)
            else:
                image, rows, res = ctx.region_components(f["depth"], f["labels"], f["K"], f["fmt"], TOL, 1)
                C.assert_same(image, rows, want[1], want[2], "components %s" % name)
            assert res.as_dict() == want[3]

        def track(f, name, where, reset=False):
            if reset:      # (the tracker's state is an image of one camera: another frame size starts over)
                trk.reset(); ref_trk.reset()
            wrc, wout, wids, wres = ref_trk.update(f["fmt"], f["depth"], f["labels"], f["K"])
            assert wrc == 0
            if where == "device":
                d = dev[name]; di = d.out(f["n"])
                trk.update(d.depth.data_ptr(), d.labels.data_ptr(), f["K"], f["fmt"], ids_out=di.data_ptr(), on_device=True)
                check = lambda: np.testing.assert_array_equal(d.get(di, np.dtype(np.uint32), f["n"]), wout, "track ids %s" % name)
                check(); held.append(check)
            else:
                np.testing.assert_array_equal(trk.update(f["depth"], f["labels"], f["K"], f["fmt"]), wout, "track ids %s" % name)
            assert np.array_equal(trk.ids(), wids)
            assert trk.result.as_dict() == wres, (trk.result.as_dict(), wres)

        def bad_label(f, call):
            lab = f["labels"].copy(); lab.reshape(-1)[f["n"] // 2] = f["K"]
            with pytest.raises(P.F3dsError) as e:
                call(lab)
            assert e.value.code == P.ERR_ARG

        table(big, "big", "host", True)
        shapes(small, "small", "device")
        boxes(big, "big", "host")
        track(big, "big", "host")
        contacts(big, "big", "device")
        components(small, "small", "host")
        table(small, "small", "device", False)
        boxes(small, "small", "device")
        track(big, "big", "device")
        shapes(big, "big", "host")
        contacts(small, "small", "host")
        components(big, "big", "device")
        # a label >= n_regions in the middle: the call fails, and every call after it is exact
        bad_label(big, lambda lab: ctx.region_shapes(big["depth"], lab, big["K"], big["fmt"]))
        bad_label(small, lambda lab: ctx.region_components(small["depth"], lab, small["K"], small["fmt"], TOL, 1))
        bad_label(big, lambda lab: trk.update(big["depth"], lab, big["K"], big["fmt"]))
        bad_label(small, lambda lab: ctx.region_boxes(small["depth"], lab, small["K"], small["fmt"]))
        table(small, "small", "host", True)
        shapes(big, "big", "device")
        boxes(small, "small", "host")
        track(small, "small", "host", reset=True)
        contacts(small, "small", "device")
        components(big, "big", "host")
        table(big, "big", "device", False)
        track(small, "small", "device")
        contacts(big, "big", "host")
        boxes(big, "big", "device")
        components(small, "small", "device")
        shapes(small, "small", "host")
        table(big, "big", "device", True)
        assert len(held) == 13
        for check in held:      # what the earlier calls left on the device is as they left it
            check()
    finally:
        trk.close(); ctx.close()


@pytest.mark.parametrize("cap", [0, 1])
def test_interleaved_calls_on_one_context(P, monkeypatch, cap):
    if P.device_count() < 1:
        pytest.fail("GPU test selected but libf3ds sees no HIP device (no CPU fallback exists)")
    if cap:
        monkeypatch.setenv("F3DS_GRID_CAP", str(cap))
    run_sequence(P)
