#!/usr/bin/env python3
"""AdaptiveWeight with fc_num 2 and 3 (csrc/adaptive_weight_mlp.hip, local_aggregation.adaptive_weight(..., fc_hidden=...)) at the ConvNet's layer shapes
(adaptive_weight_general_time.py's pyramid: N = 200 000, dl0 = 0.04, density 5, K_lim = 26,31,38,41, widths 72,144,288,576) whose M = C / shared_channels is
inside the kernels' limits (16 .. 144): shared_channels 8 at the widths 144, 288, 576 and shared_channels 1 at 72 and 144.  Modes 'dp' and 'dp_fj', masked
softmax, 'sum', relu; forward and forward + backward.
The yardstick is the same operator composed from torch ops in fp32 on the same device, in the same process: the reference's direct form (gather, concatenate,
the MLP per pair, softmax, reshape-multiply, reduction), which materialises every (n, K, .) tensor — what a user has to write without the kernels.  fc_num 1
of the same shape through the general kernels is timed beside it, so the cost of the extra layers is visible.
Medians of HIP-event timings after a warm-up, microseconds.  One JSON document on stdout.

    python tools/adaptive_weight_mlp_time.py [--layers 0,1,2,3] [--reps 11] [--no-torch]"""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from contrastboundary_amd import local_aggregation as LA, synthetic as S, tf_ops  # noqa: E402

WIDTHS = [72, 144, 288, 576]
LIMITS = [26, 31, 38, 41, 39]
SOFTMAX, REDUCTION, ACTIVATION = "dense", "sum", "relu"


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


def torch_graph_form(q, s, idx, f, radius, W, b, hidden, shared, mode):
    """the reference's formulation of 'dp' / 'dp_fj' + the layers + masked softmax + 'sum': every (n, K, .) tensor exists"""
    n0, C = f.shape
    n, K = idx.shape
    idx = idx.long()
    sf = torch.cat([f, torch.zeros_like(f[:1])])
    sp = torch.cat([s, torch.zeros_like(s[:1])])
    fj = sf[idx]
    dp = (sp[idx] - q[:, None]) / radius
    y = (torch.cat([dp, fj], -1) if mode == "dp_fj" else dp) @ W + b
    for w, v in hidden:
        y = torch.relu(y) @ w + v
    mask = (idx < n0)[..., None]
    w = torch.softmax(y.masked_fill(~mask, -1e30), 1) * mask
    return (w[..., None] * fj.reshape(n, K, C // shared, shared)).reshape(n, K, C).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="0,1,2,3")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adaptive_weight_mlp_time: no GPU (a timing needs the device)")
    dev = "cuda"
    xyz_np, _ = S.s_room(200000, 0, scale=4.0)
    pts = torch.from_numpy(xyz_np).to(dev)
    lens = torch.tensor([200000], dtype=torch.int32, device=dev)
    pyr = tf_ops.segmentation_inputs_radius(pts, lens, 0.04, 5.0, 5, LIMITS)
    rng = np.random.default_rng(3)
    r0 = 0.04 * 5.0 / 2.0
    rows = []
    for l in [int(x) for x in args.layers.split(",")]:
        C = WIDTHS[l]
        q = pyr["points"][l].contiguous()
        nb = pyr["neighbors"][l].contiguous()
        n, K = nb.shape
        radius = r0 * 2 ** l
        new = lambda *shape, scale=1.0: torch.from_numpy((rng.normal(size=shape) * scale).astype(np.float32)).to(dev)
        f = new(n, C).requires_grad_(True)
        go = new(n, C)
        for shared in (8, 1):
            M = C // shared
            if not 16 <= M <= 144:
                continue
            for mode in ("dp", "dp_fj"):
                d_in = 3 + (C if mode == "dp_fj" else 0)
                W = new(d_in, M, scale=1.0 / np.sqrt(d_in)).requires_grad_(True)
                b = new(M, scale=0.3).requires_grad_(True)
                layers = [(new(M, M, scale=1.0 / np.sqrt(M)).requires_grad_(True), new(M, scale=0.3).requires_grad_(True)) for _ in range(2)]
                for fc_num in (1, 2, 3):
                    hidden = layers[:fc_num - 1]
                    leaves = [f, W, b] + [t for pair in hidden for t in pair]

                    def fused():
                        return LA.adaptive_weight(q, q, nb, f, radius, W, b, REDUCTION, local_input_feature=mode, shared_channels=shared,
                                                  weight_softmax=SOFTMAX, fc_hidden=hidden, activation_fn=ACTIVATION)

                    def composed():
                        return torch_graph_form(q, q, nb, f, radius, W, b, hidden, shared, mode)

                    def both(fn):
                        def run():
                            for t in leaves:
                                t.grad = None
                            fn().backward(go)
                        return run

                    def forward_only(fn):
                        def run():
                            with torch.no_grad():
                                fn()
                        return run

                    r = {"layer": l, "n": n, "K": K, "C": C, "shared_channels": shared, "M": M, "mode": mode, "fc_num": fc_num,
                         "kernels": "adaptive_weight_general" if fc_num == 1 else "adaptive_weight_mlp"}
                    r["fused_fwd_us"] = timeit(forward_only(fused), args.reps)
                    r["fused_fwd_bwd_us"] = timeit(both(fused), args.reps)
                    if not args.no_torch:
                        r["torch_fwd_us"] = timeit(forward_only(composed), args.reps)
                        r["torch_fwd_bwd_us"] = timeit(both(composed), args.reps)
                        with torch.no_grad():
                            ref = composed()
                            r["max_abs_difference"] = float((fused() - ref).abs().max())
                            r["max_abs_reference"] = float(ref.abs().max())
                            del ref
                    rows.append({k: (round(v, 1) if isinstance(v, float) and k.endswith("_us") else v) for k, v in r.items()})
                    print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
                    torch.cuda.empty_cache()
        del f, go
        torch.cuda.empty_cache()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "options": "weight_softmax %s, %s, %s" % (SOFTMAX, REDUCTION, ACTIVATION),
                      "timing": "median of %d HIP-event timings after 3 warm-up calls, microseconds" % args.reps, "rows": rows}))


if __name__ == "__main__":
    main()
