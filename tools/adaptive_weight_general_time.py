#!/usr/bin/env python3
"""AdaptiveWeight through the general kernels (csrc/adaptive_weight_general.hip, local_aggregation.adaptive_weight) at the ConvNet's layer shapes
(bench_stages.py's ConvNet rows: N = 200 000, dl0 = 0.04, density 5, K_lim = 26,31,38,41, widths 72,144,288,576), forward and forward + backward:
  * 'dp_fj', shared_channels 8, masked softmax, 'sum', beside a torch composition of the same graph form that materialises the per-pair tensors (the
    reference's formulation restated: gather, concatenate, matmul, softmax, reshape-multiply, reduction);
  * the shipped configuration ('dp', shared_channels 1, no softmax, 'mean') through the general kernels, beside the kernels specialised for it, on the same
    inputs, both arms in one process.
Medians of HIP-event timings after a warm-up, microseconds; the fraction of HBM peak is taken against the ALGORITHMIC bytes of the fused operator (every
walk's gathered rows plus the per-point rows), 8 TB/s.  One JSON document on stdout.

    python tools/adaptive_weight_general_time.py [--layers 0,1,2,3] [--reps 11] [--no-torch]"""
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
MODE, SHARED, SOFTMAX, REDUCTION = "dp_fj", 8, "dense", "sum"


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


def torch_graph_form(q, s, idx, f, radius, W, b, shared):
    """the reference's formulation of 'dp_fj' + masked softmax + 'sum': every (n, K, .) tensor exists"""
    n0, C = f.shape
    n, K = idx.shape
    idx = idx.long()
    sf = torch.cat([f, torch.zeros_like(f[:1])])
    sp = torch.cat([s, torch.zeros_like(s[:1])])
    fj = sf[idx]
    dp = (sp[idx] - q[:, None]) / radius
    y = torch.cat([dp, fj], -1) @ W + b
    mask = (idx < n0)[..., None]
    w = torch.softmax(y.masked_fill(~mask, -1e30), 1) * mask
    return (w[..., None] * fj.reshape(n, K, C // shared, shared)).reshape(n, K, C).sum(1)


def algorithmic_bytes(n, K, pairs, C, M, has_nbr):
    """general kernels, `pairs` = the real entries of the table.  A query-side walk reads the n*K indices, the query points and per real pair one point and
    (feature-driven modes) one neighbor_term row of M floats; a walk that multiplies also gathers the feature row of C floats.  Forward: the softmax walk and
    the multiply walk, one output row per query.  Backward: the query side walks three times (softmax statistics; D with the feature rows; dy with the feature
    rows again and grad_out), the target side twice per real pair (grad_neighbor: grad_out row, per-query rows; grad_features_value: grad_out row again),
    each reading the query's point and per-query rows of M floats, and writes one row of C and one of M per target"""
    walk = 4 * n * K + 12 * n + 12 * pairs + (4 * pairs * M if has_nbr else 0)
    fwd = 2 * walk + 4 * pairs * C + 4 * n * C
    bwd = 3 * walk + 2 * 4 * pairs * C + 2 * 4 * n * C + 2 * 4 * n * M + 2 * (4 * pairs * C + 12 * pairs + 2 * 4 * pairs * M) + 4 * n * C + 4 * n * M
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="0,1,2,3")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adaptive_weight_general_time: no GPU (a timing needs the device)")
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
        M = C // SHARED
        q = pyr["points"][l].contiguous()
        nb = pyr["neighbors"][l].contiguous()
        n, K = nb.shape
        radius = r0 * 2 ** l
        new = lambda *shape, scale=1.0: torch.from_numpy((rng.normal(size=shape) * scale).astype(np.float32)).to(dev)
        f = new(n, C).requires_grad_(True)
        W = new(3 + C, M, scale=1.0 / np.sqrt(3 + C)).requires_grad_(True)
        b = new(M, scale=0.3).requires_grad_(True)
        W3 = new(3, C, scale=1.0 / np.sqrt(3)).requires_grad_(True)
        b3 = new(C, scale=0.3).requires_grad_(True)
        go = new(n, C)

        def fused():
            return LA.adaptive_weight(q, q, nb, f, radius, W, b, REDUCTION, local_input_feature=MODE, shared_channels=SHARED, weight_softmax=SOFTMAX)

        def composed():
            return torch_graph_form(q, q, nb, f, radius, W, b, SHARED)

        def shipped_general():                                       # the shipped configuration through the general entries
            return LA._AdaptiveWeightGeneral.apply(q, q, nb, f, None, None, W3, b3, float(radius), 0, 1)

        def shipped_present():
            return LA.adaptive_weight(q, q, nb, f, radius, W3, b3, "mean")

        def both(fn):
            def run():
                for t in (f, W, b, W3, b3):
                    t.grad = None
                fn().backward(go)
            return run

        def forward_only(fn):
            def run():
                with torch.no_grad():
                    fn()
            return run

        pairs = int((nb < n).sum())
        r = {"layer": l, "n": n, "K": K, "C": C, "M": M, "shadow_fraction": round(float((nb == n).float().mean()), 3)}
        r["fused_fwd_us"] = timeit(forward_only(fused), args.reps)
        r["fused_fwd_bwd_us"] = timeit(both(fused), args.reps)
        fb, bb = algorithmic_bytes(n, K, pairs, C, M, True)
        r["fused_fwd_hbm_fraction"] = round(fb / (r["fused_fwd_us"] * 1e-6) / HBM_PEAK, 4)
        r["fused_fwd_bwd_hbm_fraction"] = round((fb + bb) / (r["fused_fwd_bwd_us"] * 1e-6) / HBM_PEAK, 4)
        if not args.no_torch:
            r["torch_fwd_us"] = timeit(forward_only(composed), args.reps)
            r["torch_fwd_bwd_us"] = timeit(both(composed), args.reps)
            with torch.no_grad():
                r["max_abs_difference"] = float((fused() - composed()).abs().max())
        r["shipped_general_fwd_us"] = timeit(forward_only(shipped_general), args.reps)
        r["shipped_general_fwd_bwd_us"] = timeit(both(shipped_general), args.reps)
        r["shipped_present_fwd_us"] = timeit(forward_only(shipped_present), args.reps)
        r["shipped_present_fwd_bwd_us"] = timeit(both(shipped_present), args.reps)
        with torch.no_grad():
            r["shipped_max_abs_difference"] = float((shipped_general() - shipped_present()).abs().max())
        rows.append({k: (round(v, 1) if isinstance(v, float) and k.endswith("_us") else v) for k, v in r.items()})
        del f, W, b, W3, b3, go
        torch.cuda.empty_cache()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "general": "%s, shared_channels %d, weight_softmax %s, %s" % (MODE, SHARED, SOFTMAX, REDUCTION),
                      "shipped": "dp, shared_channels 1, no softmax, mean",
                      "timing": "median of %d HIP-event timings after 3 warm-up calls, microseconds" % args.reps, "layers": rows}))


if __name__ == "__main__":
    main()
