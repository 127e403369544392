#!/usr/bin/env python3
"""The ConvNet's unary layer (csrc/unary_layer.hip, contrastboundary_amd.unary.conv1d_1x1) at the shapes it has in a 200 000-point scene: the input conv, the
bottleneck convs of the five stages (rows quartered from stage to stage) and the head's first and last up_conv.  Batch statistics, relu; forward alone and
forward + backward (gradients of the features, weights, gamma and beta).
The yardstick is the same layer composed from torch ops in fp32 on the same device, in the same process: x @ w, a TF-semantics batch norm written in torch
ops (biased variance, rsqrt(var + eps), the moving update), relu.  The layer is never compared against itself.
Every variant is captured in a graph once and replayed; a sample is `--inner` replays between two device events, the variants of a shape alternate over
`--reps` rounds, the median sample is reported (microseconds per replay).  One JSON document on stdout, the rows also on stderr as they come.

    python tools/bench_unary.py [--reps 15] [--inner 10] [--only 0,3]"""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from contrastboundary_amd import unary  # noqa: E402

# (name, c_in, c_out, rows)
SHAPES = [("input conv", 5, 72, 200000), ("stage 0 conv", 72, 72, 200000), ("stage 0 -> 1", 72, 144, 200000), ("stage 1 -> 2", 144, 288, 50000),
          ("stage 2 -> 3", 288, 576, 12500), ("stage 3 -> 4", 576, 1152, 3100), ("stage 4", 1152, 2304, 800), ("head up_conv0", 3456, 576, 3100),
          ("head up_conv3", 288, 72, 200000)]
EPS, MOMENTUM = 1e-3, 0.98


def composed(x, w, gamma, beta, mm, mv):
    y = x @ w
    var, mean = torch.var_mean(y, 0, unbiased=False)
    with torch.no_grad():
        mm.mul_(MOMENTUM).add_(mean, alpha=1 - MOMENTUM)
        mv.mul_(MOMENTUM).add_(var, alpha=1 - MOMENTUM)
    return torch.relu((y - mean) * torch.rsqrt(var + EPS) * gamma + beta)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_unary: no GPU (a timing needs the device)")
    dev = "cuda"
    rng = np.random.default_rng(11)
    picked = [int(s) for s in args.only.split(",")] if args.only else range(len(SHAPES))
    rows_out = []
    for i in picked:
        name, c_in, c_out, rows = SHAPES[i]
        new = lambda *shape, scale=1.0, shift=0.0: torch.from_numpy((rng.normal(size=shape) * scale + shift).astype(np.float32)).to(dev)
        x, w = new(rows, c_in).requires_grad_(True), new(c_in, c_out, scale=1.0 / np.sqrt(c_in)).requires_grad_(True)
        gamma, beta = new(c_out, scale=0.2, shift=1.0).requires_grad_(True), new(c_out, scale=0.3).requires_grad_(True)
        go = new(rows, c_out)
        mm, mv = torch.zeros(c_out, device=dev), torch.ones(c_out, device=dev)
        leaves = [x, w, gamma, beta]
        ours = lambda: unary.conv1d_1x1(x, w, None, gamma, beta, mm, mv, is_training=True, activation_fn="relu", bn_momentum=MOMENTUM, bn_eps=EPS)
        theirs = lambda: composed(x, w, gamma, beta, mm, mv)

        def forward_only(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        def both(fn):
            return lambda: torch.autograd.grad(fn(), leaves, go)
        variants = {"layer_fwd_us": forward_only(ours), "layer_fwd_bwd_us": both(ours), "torch_fwd_us": forward_only(theirs), "torch_fwd_bwd_us": both(theirs)}
        with torch.no_grad():
            ref = theirs()
            diff, scale = float((ours() - ref).abs().max()), float(ref.abs().max())
        graphs = {k: capture(fn) for k, fn in variants.items()}
        samples = {k: [] for k in graphs}
        for _ in range(args.reps):
            for k, (g, _) in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.inner):
                    g.replay()
                e1.record()
                torch.cuda.synchronize()
                samples[k].append(e0.elapsed_time(e1) * 1e3 / args.inner)
        r = {"shape": name, "c_in": c_in, "c_out": c_out, "rows": rows}
        r.update({k: round(float(np.median(v)), 1) for k, v in samples.items()})
        r.update({k.replace("_us", "_min_us"): round(float(np.min(v)), 1) for k, v in samples.items()})
        r["fwd_layer_over_torch"] = round(r["layer_fwd_us"] / r["torch_fwd_us"], 2)
        r["fwd_bwd_layer_over_torch"] = round(r["layer_fwd_bwd_us"] / r["torch_fwd_bwd_us"], 2)
        r["max_abs_difference"], r["max_abs_reference"] = diff, scale
        rows_out.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
        del graphs, x, w, go
        torch.cuda.empty_cache()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "options": "batch statistics, relu, no bias, no shortcut",
                      "timing": "median (and minimum) of %d samples of %d graph replays each, variants alternating; microseconds per replay" % (args.reps, args.inner),
                      "rows": rows_out}))


if __name__ == "__main__":
    main()
