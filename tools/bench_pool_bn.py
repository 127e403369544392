#!/usr/bin/env python3
"""pool_bn (csrc/pool_bn.hip, contrastboundary_amd.unary.pool_bn: TF batch norm + relu behind a local aggregation) at the aggregation shapes of a real
200 000-point pyramid (convnet_path.ConvNetScene through tf_ops.segmentation_inputs_radius): the five layers' rows at C = 72, 144, 288, 576, 1152 and the
four strided aggregations (the next layer's rows at the layer's width; a five-layer pyramid has no fifth).  Batch statistics; forward alone and forward +
backward (gradients of x, gamma, beta).
The yardstick is the float32 composition a user would write in torch ops today, on the same device, in the same process: var_mean, the moving update,
normalise, relu, under autograd.  pool_bn is never compared against itself.
Algorithmic bytes: forward 12 rows C (x read for the statistics, x read and out written by the element pass); backward 28 rows C (grad_out, out and x read
by the sums pass, read again by the element pass that writes grad_x: 12 + 16) — 40 rows C for forward + backward; the share of the 8 TB/s peak is those
bytes over the measured time.
`--bottleneck`: forward + backward of one convnet_blocks.Bottleneck (adaptive_weight, width 2 C -> 2 C through C) at each
layer of the same pyramid — nothing earlier exists to compare it with: a BASELINE for later fusion work.
Every variant is captured in a graph once and replayed; a sample is `--inner` replays between two device events, the variants of a shape alternate over
`--reps` rounds, the median sample is reported (microseconds per replay).  One JSON document on stdout, the rows also on stderr as they come.

    python tools/bench_pool_bn.py [--reps 15] [--inner 10] [--points 200000] [--bottleneck]"""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from contrastboundary_amd import convnet_path as CP, tf_ops, unary  # noqa: E402

EPS, MOMENTUM, PEAK = 1e-3, 0.98, 8.0e12


def composed(x, gamma, beta, mm, mv):
    var, mean = torch.var_mean(x, 0, unbiased=False)
    with torch.no_grad():
        mm.mul_(MOMENTUM).add_(mean, alpha=1 - MOMENTUM)
        mv.mul_(MOMENTUM).add_(var, alpha=1 - MOMENTUM)
    return torch.relu((x - mean) * torch.rsqrt(var + EPS) * gamma + beta)


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    return g, keep


def time_variants(variants, reps, inner):
    """variants: name -> callable.  -> name -> (median, minimum) microseconds per replay, the variants alternating"""
    graphs = {k: capture(fn) for k, fn in variants.items()}
    samples = {k: [] for k in graphs}
    for _ in range(reps):
        for k, (g, _) in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            samples[k].append(e0.elapsed_time(e1) * 1e3 / inner)
    return {k: (round(float(np.median(v)), 2), round(float(np.min(v)), 2)) for k, v in samples.items()}


def pool_bn_case(rows, C, rng, dev):
    new = lambda *shape, scale=1.0, shift=0.0: torch.from_numpy((rng.normal(size=shape) * scale + shift).astype(np.float32)).to(dev)
    x = new(rows, C, scale=1.7, shift=0.4).requires_grad_(True)
    gamma, beta = new(C, scale=0.2, shift=1.0).requires_grad_(True), new(C, scale=0.3).requires_grad_(True)
    go = new(rows, C)
    mm, mv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    leaves = [x, gamma, beta]
    ours = lambda: unary.pool_bn(x, gamma, beta, mm, mv, is_training=True, activation_fn="relu", bn_momentum=MOMENTUM, bn_eps=EPS)
    theirs = lambda: composed(x, gamma, beta, mm, mv)

    def forward_only(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run
    both = lambda fn: (lambda: torch.autograd.grad(fn(), leaves, go))
    return ours, theirs, forward_only, both


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--bottleneck", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pool_bn: no GPU (a timing needs the device)")
    dev = "cuda"
    rng = np.random.default_rng(11)
    scene = CP.ConvNetScene(args.points)
    L = CP.NUM_LAYERS
    pyr = tf_ops.segmentation_inputs_radius(scene.points, scene.lengths, CP.DL0, CP.DENSITY, L, CP.LIMITS + [CP.LIMITS[-1]])
    sizes = [int(p.shape[0]) for p in pyr["points"]]
    shapes = [("layer %d" % l, sizes[l], CP.WIDTHS[l]) for l in range(L)] + [("strided %d -> %d" % (l, l + 1), sizes[l + 1], CP.WIDTHS[l]) for l in range(L - 1)]
    doc = {"device": torch.cuda.get_device_name(0), "points": args.points, "layer_sizes": sizes, "options": "batch statistics, relu",
           "bytes": "forward 12 rows C, backward 28 rows C (sums pass 12, element pass 16), forward + backward 40 rows C; peak 8 TB/s",
           "timing": "median (and minimum) of %d samples of %d graph replays each, variants alternating; microseconds per replay" % (args.reps, args.inner),
           "rows": [], "bottleneck": []}
    for name, rows, C in shapes:
        ours, theirs, forward_only, both = pool_bn_case(rows, C, rng, dev)
        with torch.no_grad():
            ref = theirs()
            diff, scale = float((ours() - ref).abs().max()), float(ref.abs().max())
        t = time_variants({"pool_bn_fwd": forward_only(ours), "pool_bn_fwd_bwd": both(ours), "torch_fwd": forward_only(theirs), "torch_fwd_bwd": both(theirs)},
                          args.reps, args.inner)
        r = {"shape": name, "rows": rows, "C": C}
        for k, (med, mn) in t.items():
            r[k + "_us"], r[k + "_min_us"] = med, mn
        r["fwd_over_torch"] = round(r["pool_bn_fwd_us"] / r["torch_fwd_us"], 3)
        r["fwd_bwd_over_torch"] = round(r["pool_bn_fwd_bwd_us"] / r["torch_fwd_bwd_us"], 3)
        r["fwd_share_of_peak"] = round(12.0 * rows * C / (r["pool_bn_fwd_us"] * 1e-6) / PEAK, 4)
        r["fwd_bwd_share_of_peak"] = round(40.0 * rows * C / (r["pool_bn_fwd_bwd_us"] * 1e-6) / PEAK, 4)
        r["max_abs_difference"], r["max_abs_reference"] = diff, scale
        doc["rows"].append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    if args.bottleneck:
        from contrastboundary_amd import convnet_blocks as B
        r0 = CP.DL0 * CP.DENSITY / 2
        for l in range(L):
            W = CP.WIDTHS[l]
            torch.manual_seed(l)
            m = B.Bottleneck(l, 2 * W, 2 * W, 2, r0 * 2 ** l, dict(kind="adaptive_weight")).to(dev)
            f = torch.from_numpy(rng.normal(size=(sizes[l], 2 * W)).astype(np.float32)).to(dev).requires_grad_(True)
            go = torch.from_numpy(rng.normal(size=(sizes[l], 2 * W)).astype(np.float32)).to(dev)
            leaves = [f] + list(m.parameters())
            t = time_variants({"fwd_bwd": lambda: torch.autograd.grad(m(pyr, f), leaves, go)}, args.reps, args.inner)
            r = {"layer": l, "rows": sizes[l], "width": 2 * W, "mid": W, "neighbors": int(pyr["neighbors"][l].shape[1]), "fwd_bwd_us": t["fwd_bwd"][0],
                 "fwd_bwd_min_us": t["fwd_bwd"][1]}
            doc["bottleneck"].append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
            del m, f, go
            torch.cuda.empty_cache()
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
