#!/usr/bin/env python3
"""The segmentation head's four decoder steps (contrastboundary_amd.unary.up_conv over cbl_up_conv_*, csrc/up_conv.hip) at the shapes they
have at fdim 72 in a 200 000-point scene: up_conv0 2304 + 1152 -> 576 onto layer 3, up_conv1 576 + 576 -> 288 onto layer 2, up_conv2 288 + 288 -> 144 onto
layer 1, up_conv3 144 + 144 -> 72 onto layer 0.  Batch statistics, relu; forward alone and forward + backward (gradients of the coarse and the skip features,
the weights, gamma and beta).  The row counts and the upsample tables are those of a real grid pyramid (convnet_path.ConvNetScene's cloud through
tf_ops.segmentation_inputs_radius: dl0 0.04, density 5, the S3DIS neighbourhood limits).
`--rows nominal` runs the same widths at the row counts of a pyramid that quarters from layer to layer — (3 100, 800), (12 500, 3 100), (50 000, 12 500),
(200 000, 50 000) — with a table that sends fine row i to coarse row floor(i n1 / n2): not a real pyramid, but the shapes at which the coarse layer's
products are small (800 x 2304 -> 576: 117 tiles), which is where the split of their contraction (ul_split_of) applies; `--split-ab` adds the fused variants
with that split switched off (CBL_UP_CONV_SPLIT=0 while they are captured).
The yardstick is the same step composed from the library's existing entries, with the upsampled and the concatenated tensor:
conv1d_1x1(cat(nearest_upsample(coarse, inds), skip)).  Both variants run in this process as captured graphs; the transposed table of each upsample table is
built once, before any capture, and serves both.  A sample is `--inner` replays between two device events, the variants of a shape alternate over `--reps`
rounds; reported are the median, the minimum and the interquartile range of the samples (microseconds per replay) and the ratio of the medians.  One JSON
document on stdout, the rows also on stderr as they come.

    python tools/bench_up_conv.py [--reps 21] [--inner 10] [--only 0,3] [--n 200000] [--rows pyramid|nominal] [--split-ab]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from contrastboundary_amd import convnet_path, local_aggregation, pointops, tf_ops, unary  # noqa: E402
from contrastboundary_amd.local_aggregation import first_column  # noqa: E402

FDIM = 72
# (name, the finer layer, c_up, c_skip, c_out)
STEPS = [("up_conv0", 3, 32 * FDIM, 16 * FDIM, 8 * FDIM), ("up_conv1", 2, 8 * FDIM, 8 * FDIM, 4 * FDIM), ("up_conv2", 1, 4 * FDIM, 4 * FDIM, 2 * FDIM),
         ("up_conv3", 0, 2 * FDIM, 2 * FDIM, FDIM)]
NOMINAL = {3: (3100, 800), 2: (12500, 3100), 1: (50000, 12500), 0: (200000, 50000)}      # the finer layer -> (n2, n1)
EPS, MOMENTUM = 1e-3, 0.98


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
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--rows", choices=("pyramid", "nominal"), default="pyramid")
    ap.add_argument("--split-ab", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_up_conv: no GPU (a timing needs the device)")
    dev = "cuda"
    if args.rows == "pyramid":
        scene = convnet_path.ConvNetScene(args.n, seed=0)
        pyr = tf_ops.segmentation_inputs_radius(scene.points, scene.lengths, convnet_path.DL0, convnet_path.DENSITY, 5, convnet_path.LIMITS)
    rng = np.random.default_rng(12)
    picked = [int(s) for s in args.only.split(",")] if args.only else range(len(STEPS))
    rows_out = []
    for i in picked:
        name, fine, c_up, c_skip, c_out = STEPS[i]
        if args.rows == "pyramid":
            inds = pyr["upsamples"][fine + 1].contiguous()
            n2, n1 = pyr["points"][fine].shape[0], pyr["points"][fine + 1].shape[0]
        else:
            n2, n1 = NOMINAL[fine]
            inds = (torch.arange(n2, device=dev, dtype=torch.int64) * n1 // n2).to(torch.int32).reshape(n2, 1).contiguous()
        assert inds.shape[0] == n2
        new = lambda *shape, scale=1.0, shift=0.0: torch.from_numpy((rng.normal(size=shape) * scale + shift).astype(np.float32)).to(dev)
        coarse, skip = new(n1, c_up).requires_grad_(True), new(n2, c_skip).requires_grad_(True)
        w = new(c_up + c_skip, c_out, scale=1.0 / np.sqrt(c_up + c_skip)).requires_grad_(True)
        gamma, beta = new(c_out, scale=0.2, shift=1.0).requires_grad_(True), new(c_out, scale=0.3).requires_grad_(True)
        go = new(n2, c_out)
        mm, mv = torch.zeros(c_out, device=dev), torch.ones(c_out, device=dev)
        leaves = [coarse, skip, w, gamma, beta]
        kw = dict(is_training=True, activation_fn="relu", bn_momentum=MOMENTUM, bn_eps=EPS)
        fused = lambda: unary.up_conv(coarse, inds, skip, w, None, gamma, beta, mm, mv, **kw)
        composed = lambda: unary.conv1d_1x1(torch.cat([local_aggregation.nearest_upsample(coarse, inds), skip], 1), w, None, gamma, beta, mm, mv, **kw)
        # the transposed table both backward passes walk: built here, once, and found in the registry afterwards (as in a training loop)
        assert pointops.neighbor_transpose(first_column(inds), n1, build=True) is not None

        def forward_only(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        def both(fn):
            return lambda: torch.autograd.grad(fn(), leaves, go)
        variants = {"fused_fwd_us": forward_only(fused), "composed_fwd_us": forward_only(composed), "fused_fwd_bwd_us": both(fused),
                    "composed_fwd_bwd_us": both(composed)}
        if args.split_ab:
            variants.update({"fused_nosplit_fwd_us": forward_only(fused), "fused_nosplit_fwd_bwd_us": both(fused)})
        with torch.no_grad():
            ref = composed()
            diff, scale = float((fused() - ref).abs().max()), float(ref.abs().max())
        ga, gb = both(fused)(), both(composed)()
        grad_diff = max(float((a - b).norm() / b.norm()) for a, b in zip(ga, gb))         # (relu masks within rounding of zero differ between two fp32 forms)
        del ga, gb, ref
        graphs = {}
        for key, fn in variants.items():                             # the knob is read when a call is issued, which for a graph is its capture
            os.environ["CBL_UP_CONV_SPLIT"] = "0" if "nosplit" in key else "1"
            graphs[key] = capture(fn)
        os.environ.pop("CBL_UP_CONV_SPLIT")
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
        r = {"step": name, "n2": n2, "n1": n1, "k": inds.shape[1], "c_up": c_up, "c_skip": c_skip, "c_out": c_out,
             "shadow_fraction": round(float(((inds[:, 0] < 0) | (inds[:, 0] >= n1)).float().mean()), 4)}
        r.update({k: round(float(np.median(v)), 1) for k, v in samples.items()})
        r.update({k.replace("_us", "_min_us"): round(float(np.min(v)), 1) for k, v in samples.items()})
        r.update({k.replace("_us", "_iqr_us"): round(float(np.percentile(v, 75) - np.percentile(v, 25)), 1) for k, v in samples.items()})
        r["fwd_fused_over_composed"] = round(r["fused_fwd_us"] / r["composed_fwd_us"], 3)
        r["fwd_bwd_fused_over_composed"] = round(r["fused_fwd_bwd_us"] / r["composed_fwd_bwd_us"], 3)
        if args.split_ab:
            r["fwd_split_over_nosplit"] = round(r["fused_fwd_us"] / r["fused_nosplit_fwd_us"], 3)
            r["fwd_bwd_split_over_nosplit"] = round(r["fused_fwd_bwd_us"] / r["fused_nosplit_fwd_bwd_us"], 3)
        r["max_abs_difference"], r["max_abs_reference"], r["max_rel_l2_grad_difference"] = diff, scale, grad_diff
        rows_out.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
        del graphs, coarse, skip, w, go
        torch.cuda.empty_cache()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "options": "batch statistics, relu, no bias; " + ("the pyramid of n = %d points" % args.n if args.rows == "pyramid" else "nominal rows"),
                      "timing": "median, minimum and interquartile range of %d samples of %d graph replays each, variants alternating; microseconds per replay"
                                % (args.reps, args.inner), "rows": rows_out}))


if __name__ == "__main__":
    main()
