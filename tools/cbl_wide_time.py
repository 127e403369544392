#!/usr/bin/env python3
"""CBL head (heads.point_contrast, csrc/cbl_pairs.hip) at the widths of the features it may contrast: the Point Transformer's five stage outputs
(n, nsample, d) = (40960, 36, 32) (10240, 24, 64) (2560, 24, 128) (640, 24, 256) (160, 24, 512) and the 13-wide S3DIS logits at stage 0.
Forward alone (no gradient: the pass-A kernel without coefficients) and forward + backward (pass A with coefficients, pass B over the transposed
neighbour table) as hipGraph replays between HIP events, the table built before capture.  Synthetic S-room scene per stage (labels with boundaries),
random features.  python tools/cbl_wide_time.py -> one JSON line (us per replay)."""
import json
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from contrastboundary_amd import heads, pointops, synthetic as S  # noqa: E402

SHAPES = [("stage0_f_out", 40960, 36, 32), ("stage1_f_out", 10240, 24, 64), ("stage2_f_out", 2560, 24, 128), ("stage3_f_out", 640, 24, 256),
          ("stage4_f_out", 160, 24, 512), ("stage0_logits", 40960, 36, 13)]


def graph_us(fn, reps=50):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn(); fn(); fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        fn()
    ts = []
    with torch.cuda.stream(s):
        g.replay()
        for _ in range(3):                                             # median of three rounds of `reps` replays
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                g.replay()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) / reps * 1e3)
    return round(float(np.median(ts)), 1)


def main():
    out = {"device": torch.cuda.get_device_name(0)}
    for name, n, k, d in SHAPES:
        xyz_np, lab_np = S.s_room(n, seed=1)
        xyz = torch.from_numpy(xyz_np).cuda()
        lab = torch.from_numpy(lab_np.astype(np.int64)).cuda()
        off = torch.tensor([n // 2, n], dtype=torch.int32, device="cuda")
        idx, _ = pointops.knnquery_raw(k, xyz, xyz, off, off, algo="set")
        feat = torch.randn(n, d, device="cuda")
        f_grad = feat.clone().requires_grad_(True)
        pointops.neighbor_transpose(idx, n)                            # the transposed table: registered before capture, found by the backward
        keep = {}

        def fwd():
            keep["loss"] = heads.point_contrast(feat, lab, idx, 1.0, 0.1)

        def fwd_bwd():
            loss = heads.point_contrast(f_grad, lab, idx, 1.0, 0.1)
            keep["grad"] = torch.autograd.grad(loss, f_grad)[0]

        r = {"n": n, "nsample": k, "d": d, "fwd_us": graph_us(fwd), "fwd_bwd_us": graph_us(fwd_bwd)}
        r["bwd_us"] = round(r["fwd_bwd_us"] - r["fwd_us"], 1)
        r["loss"] = float(keep["loss"].item())
        out[name] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
