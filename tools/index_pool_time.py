#!/usr/bin/env python3
"""ind_max_pool / ind_closest_pool (local_aggregation over csrc/local_aggregation.hip, csrc/index_pool.hip and the transposed table) at the pooling and
upsampling shapes of the ConvNet pyramid (N = 200 000 S-room, dl0 = 0.04, density 5, K_lim = 26,31,38,41,39, widths 72,144,288,576,1152; the pyramid
convnet_path.ConvNetScene's step runs on), forward and forward + backward, beside the torch composition of the graph form under autograd
(cat / index / amax, cat / index) in the same process.  Medians of HIP-event timings after a warm-up, microseconds.  The backward's transposed table is
built once per table (the pyramid's tables do not change between steps) and found in the registry afterwards, as in a training loop.  One JSON document on stdout.

    python tools/index_pool_time.py [--layers 0,1,2,3] [--reps 11] [--no-torch]"""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from contrastboundary_amd import local_aggregation as LA, synthetic as S, tf_ops  # noqa: E402

WIDTHS = [72, 144, 288, 576, 1152]
LIMITS = [26, 31, 38, 41, 39]


def timeit(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts))


def torch_max_pool(x, inds):
    return torch.cat([x, x.amin(0, keepdim=True)])[inds].amax(1)


def torch_closest_pool(x, inds):
    return torch.cat([x, torch.zeros_like(x[:1])])[inds[:, 0]]


def measure(fused, composed, x, inds, go, reps, with_torch):
    """inds: int32 for the fused operator; the composition indexes with the same table as int64 (converted outside the timing)"""
    long_inds = inds.long()

    def forward_only(fn, table):
        def run():
            with torch.no_grad():
                fn(x, table)
        return run

    def both(fn, table):
        def run():
            x.grad = None
            fn(x, table).backward(go)
        return run
    r = {"fused_fwd_us": timeit(forward_only(fused, inds), reps), "fused_fwd_bwd_us": timeit(both(fused, inds), reps)}
    if with_torch:
        r["torch_fwd_us"] = timeit(forward_only(composed, long_inds), reps)
        r["torch_fwd_bwd_us"] = timeit(both(composed, long_inds), reps)
        both(fused, inds)(); a = x.grad.clone()
        both(composed, long_inds)(); b = x.grad
        r["max_abs_grad_difference"] = float((a - b).abs().max())
        r["max_abs_grad"] = float(b.abs().max())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="0,1,2,3")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("index_pool_time: no GPU (a timing needs the device)")
    dev = "cuda"
    xyz_np, _ = S.s_room(200000, 0, scale=4.0)
    pts = torch.from_numpy(xyz_np).to(dev)
    lens = torch.tensor([200000], dtype=torch.int32, device=dev)
    pyr = tf_ops.segmentation_inputs_radius(pts, lens, 0.04, 5.0, 5, LIMITS)
    rng = np.random.default_rng(3)
    rows = []
    for l in [int(v) for v in args.layers.split(",")]:
        # pooling: layer l's features (ReLU outputs: half of them exact zeros) onto layer l + 1;  upsampling: layer l + 1's features back onto layer l
        pool = pyr["pools"][l].contiguous()
        up = pyr["upsamples"][l + 1].contiguous()
        n1, n2 = pyr["points"][l].shape[0], pyr["points"][l + 1].shape[0]
        assert pool.shape[0] == n2 and up.shape[0] == n1
        for op, inds, src, dst, C in (("ind_max_pool", pool, n1, n2, WIDTHS[l]), ("ind_closest_pool", up, n2, n1, WIDTHS[l + 1])):
            x = torch.from_numpy(np.maximum(rng.normal(size=(src, C)), 0).astype(np.float32)).to(dev).requires_grad_(True)
            go = torch.from_numpy(rng.normal(size=(dst, C)).astype(np.float32)).to(dev)
            fused, composed = (LA.ind_max_pool, torch_max_pool) if op == "ind_max_pool" else (LA.ind_closest_pool, torch_closest_pool)
            r = {"op": op, "layer": l, "n1": src, "n2": dst, "k": inds.shape[1], "d": C, "shadow_fraction": round(float((inds == src).float().mean()), 3)}
            r.update(measure(fused, composed, x, inds, go, args.reps, not args.no_torch))
            rows.append({k: (round(v, 1) if isinstance(v, float) and k.endswith("_us") else v) for k, v in r.items()})
            del x, go
            torch.cuda.empty_cache()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "timing": "median of %d HIP-event timings after 3 warm-up calls, microseconds" % args.reps,
                      "rows": rows}))


if __name__ == "__main__":
    main()
