"""The copy-stream plumbing beside f3ds_segment (test_gpu_parity.py covers that one): the host outputs of f3ds_labels_at_thresholds_batch and the host
inputs and outputs of f3ds_tracker_update travel on the call's own stream (F3DS_COPY_STREAM=0), on the device's copy stream (1, the default) or on the
two copy streams (2).  Every setting must give the same bytes, and the bytes of the device-to-device form of the call.  One frame, the one of smoke():
synth_frame(0, 7, 160, 120, 30) at voxel_res 0.02, seed_res 0.2."""
import numpy as np
import pytest

from rgbd_common import frame_images

pytestmark = pytest.mark.gpu
SETTINGS = ("0", "1", "2")
N = 160 * 120


def params(P):
    return P.launch_params(voxel_res=0.02, seed_res=0.2)


def device_u32(n):
    import torch
    return torch.zeros(n, dtype=torch.int32, device="cuda")


def host_u32(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def test_levels_to_host_under_every_copy_stream_setting(P, monkeypatch):
    pts = P.synth_frame(0, 7, 160, 120, 30)
    ts = [0.05, 0.12, 0.2]
    ctxs = [P.Context(0) for _ in range(2)]
    try:
        seg = P.segment_batch(ctxs, [pts, pts], params(P))
        runs = {}
        for s in SETTINGS:
            monkeypatch.setenv("F3DS_COPY_STREAM", s)
            out = [np.full((len(ts), N), 0x5A5A5A5A, np.uint32) for _ in ctxs]
            labels, nreg = P.labels_at_thresholds_batch(ctxs, ts, out=out)
            runs[s] = ([l.copy() for l in labels], nreg.copy())
        monkeypatch.delenv("F3DS_COPY_STREAM")
        dev = [device_u32(len(ts) * N) for _ in ctxs]
        _, dev_nreg = P.labels_at_thresholds_batch(ctxs, ts, out=dev, on_device=True)
        dev_labels = [host_u32(d).reshape(len(ts), N) for d in dev]
        for s in SETTINGS:
            labels, nreg = runs[s]
            assert nreg.tobytes() == dev_nreg.tobytes() and nreg.shape == (2, len(ts)), s
            for i in range(2):
                assert labels[i].tobytes() == dev_labels[i].tobytes(), (s, i)
                assert np.array_equal(labels[i][-1], seg[i]), (s, i)      # (the level at the cluster run's own threshold is that run's labelling)
        assert dev_nreg[0][0] > dev_nreg[0][-1]                           # (the levels are not all one segmentation)
    finally:
        for c in ctxs:
            c.close()


def test_tracker_from_host_under_every_copy_stream_setting(P, gpu_ctx, monkeypatch):
    fmt, depth, color = frame_images(P, 7, 160, 120)
    one = P.default_track_params(min_votes=1)
    lab = gpu_ctx.segment_rgbd(depth, color, fmt, params(P))
    K = gpu_ctx.result.n_regions
    second = np.where(lab == 0, np.uint32(P.NO_LABEL), lab)      # the second frame loses a region: its ids still come from the first frame's
    frames = [lab, second]
    runs = {}
    for s in SETTINGS:
        monkeypatch.setenv("F3DS_COPY_STREAM", s)
        with P.Tracker(0, one) as trk:
            runs[s] = []
            for l in frames:
                ids = trk.update(depth, l, K, fmt, ids_out=np.full(N, 0x5A5A5A5A, np.uint32))
                runs[s].append((ids.copy(), trk.ids(), trk.result.as_dict()))
    monkeypatch.delenv("F3DS_COPY_STREAM")
    import torch
    dd = torch.from_numpy(depth.view(np.uint8).reshape(-1).copy()).cuda()
    di = device_u32(N)
    with P.Tracker(0, one) as trk:
        for f, l in enumerate(frames):
            dl = torch.from_numpy(l.view(np.int32).copy()).cuda()
            torch.cuda.synchronize()
            trk.update(dd.data_ptr(), dl.data_ptr(), K, fmt, ids_out=di.data_ptr(), on_device=True)
            want = (host_u32(di), trk.ids(), trk.result.as_dict())
            for s in SETTINGS:
                got = runs[s][f]
                assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2], (s, f)
    first, last = runs["1"][0], runs["1"][1]
    assert K > 10 and first[2]["first_frame"] == 1 and last[2]["n_new"] == 0 and last[2]["n_matched"] == last[2]["n_nonempty"] == first[2]["n_nonempty"] - 1
