#!/usr/bin/env python3
"""PointWiseMLP (csrc/pointwise_mlp.hip through local_aggregation.pointwise_mlp) at the ConvNet's layer shapes (bench_stages.py's ConvNet rows: N = 200 000,
dl0 = 0.04, density 5, K_lim = 26,31,38,41, widths 72,144,288,576), forward and forward + backward, training-mode batch norm, beside a torch composition of
the same graph form that materialises the per-pair tensors (the reference's formulation restated: gather, concatenate, matmul, batch norm, activation, mask,
reduction).  Medians of HIP-event timings after a warm-up, microseconds; the fraction of HBM peak is taken against the ALGORITHMIC bytes of the fused operator
(the K * C_out-row gathers per pass plus the per-point rows), 8 TB/s.  One JSON document on stdout.

    python tools/pointwise_mlp_time.py [--layers 0,1,2,3] [--mode dp_fj] [--reduction max] [--activation relu] [--reps 11] [--no-torch]"""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from contrastboundary_amd import local_aggregation as LA, synthetic as S, tf_ops  # noqa: E402

HBM_PEAK = 8.0e12                                                    # bytes / s
WIDTHS = [72, 144, 288, 576]
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


def torch_graph_form(q, s, idx, f, radius, W, gamma, beta, mode, reduction, activation, eps=1e-3):
    """the reference's formulation: every (n, K, .) tensor exists"""
    n0 = f.shape[0]
    K = idx.shape[1]
    idx = idx.long()
    sf = torch.cat([f, torch.zeros_like(f[:1])])
    sp = torch.cat([s, torch.zeros_like(s[:1])])
    fj = sf[idx]
    dp = (sp[idx] - q[:, None]) / radius
    if mode == "dp_fj":
        x = torch.cat([dp, fj], -1)
    else:
        fi = sf[idx[:, :1]].expand(-1, K, -1)
        x = torch.cat({"fi_df": [fi, fj - fi], "dp_fi_df": [dp, fi, fj - fi], "dp_fi_df_fj": [dp, fi, fj - fi, fj]}[mode], -1)
    y = x @ W
    mean, var = y.mean((0, 1)), y.var((0, 1), unbiased=False)
    z = (y - mean) * torch.rsqrt(var + eps) * gamma + beta
    a = torch.relu(z) if activation == "relu" else torch.nn.functional.leaky_relu(z, 0.2) if activation == "leaky_relu" else z
    a = a * (idx < n0).to(a.dtype)[..., None]
    if reduction == "max":
        return a.amax(1)
    if reduction == "sum":
        return a.sum(1)
    return a.sum(1) / ((idx < idx.max()).to(a.dtype).sum(-1, keepdim=True) + 1e-5)


def algorithmic_bytes(n, K, pairs, C_out, center):
    """fused operator, `pairs` = the real (non-shadow) entries of the table: a query-side pass gathers one row of C_out floats and one point per real pair, reads
    the n*K indices, the query points (and the centre rows); the two forward passes (statistics, apply) write one output row per query; the backward runs two
    query-side passes (reading grad_out, the second writing the centre gradient) and the target-side pass, which reads the gradient row of every real pair
    and writes one row per target"""
    qpass = 4 * pairs * C_out + 12 * pairs + 4 * n * K + 12 * n + (4 * n * C_out if center else 0)
    fwd = 2 * qpass + 4 * n * C_out
    bwd = 2 * (qpass + 4 * n * C_out) + (4 * n * C_out if center else 0) + 4 * pairs * C_out + 4 * pairs + 4 * n * C_out
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="0,1,2,3")
    ap.add_argument("--mode", default="dp_fj", choices=LA.POINTWISE_MLP_INPUTS)
    ap.add_argument("--reduction", default="max")
    ap.add_argument("--activation", default="relu")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointwise_mlp_time: no GPU (a timing needs the device)")
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
        d_in = 3 * args.mode.startswith("dp") + 2 * C * ("fi_df" in args.mode) + C * args.mode.endswith("fj")
        f = torch.from_numpy(rng.normal(size=(n, C)).astype(np.float32)).to(dev).requires_grad_(True)
        W = torch.from_numpy((rng.normal(size=(d_in, C)) / np.sqrt(d_in)).astype(np.float32)).to(dev).requires_grad_(True)
        gamma = torch.ones(C, device=dev, requires_grad=True)
        beta = torch.zeros(C, device=dev, requires_grad=True)
        go = torch.from_numpy(rng.normal(size=(n, C)).astype(np.float32)).to(dev)
        kw = dict(local_input_feature=args.mode, reduction=args.reduction, activation_fn=args.activation)

        def fused():
            return LA.pointwise_mlp(q, q, nb, f, radius, W, gamma, beta, **kw)

        def composed():
            return torch_graph_form(q, q, nb, f, radius, W, gamma, beta, args.mode, args.reduction, args.activation)

        def both(fn):
            def run():
                for t in (f, W, gamma, beta):
                    t.grad = None
                fn().backward(go)
            return run

        def forward_only(fn):
            def run():
                with torch.no_grad():
                    fn()
            return run

        r = {"layer": l, "n": n, "K": K, "C": C, "C_out": C, "shadow_fraction": round(float((nb == n).float().mean()), 3)}
        r["fused_fwd_us"] = timeit(forward_only(fused), args.reps)
        r["fused_fwd_bwd_us"] = timeit(both(fused), args.reps)
        fb, bb = algorithmic_bytes(n, K, int((nb < n).sum()), C, "fi_df" in args.mode)
        r["fused_fwd_hbm_fraction"] = round(fb / (r["fused_fwd_us"] * 1e-6) / HBM_PEAK, 4)
        r["fused_fwd_bwd_hbm_fraction"] = round((fb + bb) / (r["fused_fwd_bwd_us"] * 1e-6) / HBM_PEAK, 4)
        if not args.no_torch:
            r["torch_fwd_us"] = timeit(forward_only(composed), args.reps)
            r["torch_fwd_bwd_us"] = timeit(both(composed), args.reps)
            with torch.no_grad():
                a, b = fused(), composed()
            r["max_abs_difference"] = float((a - b).abs().max())
        rows.append({k: (round(v, 1) if isinstance(v, float) and k.endswith("_us") else v) for k, v in r.items()})
    print(json.dumps({"device": torch.cuda.get_device_name(0), "mode": args.mode, "reduction": args.reduction, "activation": args.activation,
                      "timing": "median of %d HIP-event timings after 3 warm-up calls, microseconds" % args.reps, "layers": rows}))


if __name__ == "__main__":
    main()
