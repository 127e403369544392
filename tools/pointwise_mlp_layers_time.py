#!/usr/bin/env python3
"""PointWiseMLP with fc_num 2 and 3 (csrc/pointwise_mlp_layers.hip, local_aggregation.pointwise_mlp(..., fc_hidden=...)) at the ConvNet's layer shapes
(adaptive_weight_general_time.py's pyramid: N = 200 000, dl0 = 0.04, density 5, K_lim = 26,31,38,41) with the bottleneck widths C = C_out = 36, 72, 144, 288
(half the stage widths), i.e. hidden widths H = 18, 36, 72, 144: all inside the kernels' limits.  'dp_fj', 'max', relu, batch statistics; forward and
forward + backward.
The yardsticks: the same operator composed from torch ops in fp32 on the same device, in the same process — the reference's direct form (gather, concatenate,
per layer `@ W`, batch norm over all n K rows, relu; mask, max), which materialises every (n, K, .) tensor — and fc_num 1 of the same shape through the
existing kernels (csrc/pointwise_mlp.hip), so the cost of the extra layers is visible.
Medians of HIP-event timings after a warm-up, microseconds.  One JSON document on stdout.

    python tools/pointwise_mlp_layers_time.py [--layers 0,1,2,3] [--reps 7] [--no-torch]"""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from contrastboundary_amd import local_aggregation as LA, synthetic as S, tf_ops  # noqa: E402

WIDTHS = [36, 72, 144, 288]
LIMITS = [26, 31, 38, 41, 39]
MODE, REDUCTION, ACTIVATION = "dp_fj", "max", "relu"


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


def torch_graph_form(q, s, idx, f, radius, layers, eps=1e-3):
    """the reference's formulation of 'dp_fj' + the layers with batch statistics + relu + mask + 'max': every (n, K, .) tensor exists"""
    n0 = f.shape[0]
    idx = idx.long()
    sf = torch.cat([f, torch.zeros_like(f[:1])])
    sp = torch.cat([s, torch.zeros_like(s[:1])])
    x = torch.cat([(sp[idx] - q[:, None]) / radius, sf[idx]], -1)
    for W, gamma, beta in layers:
        y = x @ W
        var, mean = torch.var_mean(y, (0, 1), unbiased=False)
        x = torch.relu((y - mean) * torch.rsqrt(var + eps) * gamma + beta)
    return (x * (idx < n0)[..., None]).amax(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="0,1,2,3")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointwise_mlp_layers_time: no GPU (a timing needs the device)")
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
        H = max(C // 2, 9)
        q = pyr["points"][l].contiguous()
        nb = pyr["neighbors"][l].contiguous()
        n, K = nb.shape
        radius = r0 * 2 ** l
        new = lambda *shape, scale=1.0, shift=0.0: torch.from_numpy((rng.normal(size=shape) * scale + shift).astype(np.float32)).to(dev)
        f = new(n, C).requires_grad_(True)
        go = new(n, C)
        for fc_num in (1, 2, 3):
            ins = [3 + C] + [H] * (fc_num - 1)
            outs = [H] * (fc_num - 1) + [C]
            layers = [(new(i, o, scale=1.0 / np.sqrt(i)).requires_grad_(True), new(o, scale=0.2, shift=1.0).requires_grad_(True),
                       new(o, scale=0.3).requires_grad_(True)) for i, o in zip(ins, outs)]
            moving = [(torch.zeros(o, device=dev), torch.ones(o, device=dev)) for o in outs]
            leaves = [f] + [t for layer in layers for t in layer]
            hidden = [layers[k] + moving[k] for k in range(1, fc_num)]

            def fused():
                return LA.pointwise_mlp(q, q, nb, f, radius, *layers[0], *moving[0], local_input_feature=MODE, reduction=REDUCTION,
                                        activation_fn=ACTIVATION, is_training=True, fc_hidden=hidden)

            def composed():
                return torch_graph_form(q, q, nb, f, radius, layers)

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

            r = {"layer": l, "n": n, "K": K, "C": C, "H": H if fc_num > 1 else None, "fc_num": fc_num,
                 "kernels": "pointwise_mlp" if fc_num == 1 else "pointwise_mlp_layers"}
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
    print(json.dumps({"device": torch.cuda.get_device_name(0), "options": "%s, %s, %s, batch statistics" % (MODE, REDUCTION, ACTIVATION),
                      "timing": "median of %d HIP-event timings after 3 warm-up calls, microseconds" % args.reps, "rows": rows}))


if __name__ == "__main__":
    main()
