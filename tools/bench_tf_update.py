"""the TF-side parameter update `tf_train.TFMomentum.clip_and_step` (cbl_tf_clip_update, csrc/tf_update.hip: per-variable clip + momentum step with the
weight decay folded in, a norm sweep plus one apply sweep) on the REAL variable list — ResnetBackbone(5, r, 72, 2, 1, adaptive_weight) plus
ResnetSceneSegmentationHead(72, 13), built from the package's modules — and on a second list of the same total cut into equal 64 K segments, beside a
torch composition of the same math written with torch._foreach_* in the same process.  Every variant is a replayed graph; the variants alternate inside a
round and the order is reversed every other round; median / minimum / interquartile range in us per replay, the fraction of the 8 TB/s peak for the
algorithmic 28 B per element, and the fused path's sweeps one by one (clip alone, step alone).  At 74 MB per buffer the three buffers fit the 256 MB
Infinity Cache: the fraction is NOT a fraction of HBM bandwidth.

    python tools/bench_tf_update.py [--rounds 30] [--replays 20]  -> one JSON line (profiles/tf_update_device.md)"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8e12                                                          # B/s (MI355X HBM3E)
LR, MOMENTUM, GRAD_NORM, WD = 0.01, 0.98, 100.0, 0.001               # config/s3dis.py


def real_list():
    from contrastboundary_amd import tf_train
    from contrastboundary_amd.convnet_blocks import ResnetBackbone
    from contrastboundary_amd.seg_head import ResnetSceneSegmentationHead
    modules = [ResnetBackbone(5, 0.1, 72, 2, 1, {"kind": "adaptive_weight"}), ResnetSceneSegmentationHead(72, 13)]
    return [(p.numel(), WD if d else 0.0) for _, p, d in tf_train.tf_variables(*modules)]


def equal_list(total, seg=65536):
    sizes = [seg] * (total // seg) + ([total % seg] if total % seg else [])
    return [(s, WD if i % 2 == 0 else 0.0) for i, s in enumerate(sizes)]


def fill(tensors, seed, scale):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for t in tensors:
        t.copy_(torch.randn(t.shape, generator=g, device="cuda") * scale)


class Fused:
    def __init__(self, variables):
        from contrastboundary_amd import tf_train
        self.params = [torch.nn.Parameter(torch.empty(n, device="cuda")) for n, _ in variables]
        self.opt = tf_train.TFMomentum(self.params, lr=LR, momentum=MOMENTUM, grad_norm=GRAD_NORM, coefficients=[c for _, c in variables], fold_decay=True)
        self.opt.mark_produced(True)
        fill([self.opt.flat_param], 1, 0.05); fill([self.opt.flat_grad], 2, 0.01)

    def variants(self):
        return {"fused clip_and_step": self.opt.clip_and_step, "fused clip alone": self.opt.clip, "fused step alone": self.opt.step}


class Foreach:
    """the same update from torch._foreach_* ops over per-variable tensors: h = g + wd w (decayed variables), per-variable norms, g' = h * (clip / max(norm,
    clip)), a = momentum a + g', w -= lr a — about 44 B per element in six multi-tensor passes (the clip as one multiply by a per-variable factor: the form of
    tf.clip_by_norm costs a pass more)"""

    def __init__(self, variables):
        self.w = [torch.empty(n, device="cuda") for n, _ in variables]
        self.g = [torch.empty(n, device="cuda") for n, _ in variables]
        self.a = [torch.zeros(n, device="cuda") for n, _ in variables]
        fill(self.w, 1, 0.05); fill(self.g, 2, 0.01)
        self.decayed = [i for i, (_, c) in enumerate(variables) if c]
        self.clip = torch.tensor(GRAD_NORM, device="cuda")

    def step(self):
        torch._foreach_add_([self.g[i] for i in self.decayed], [self.w[i] for i in self.decayed], alpha=WD)
        norms = torch._foreach_norm(self.g)
        factors = torch._foreach_div(torch._foreach_maximum(norms, GRAD_NORM), GRAD_NORM)
        torch._foreach_reciprocal_(factors)
        torch._foreach_mul_(self.g, factors)
        torch._foreach_mul_(self.a, MOMENTUM)
        torch._foreach_add_(self.a, self.g)
        torch._foreach_add_(self.w, self.a, alpha=-LR)

    def variants(self):
        return {"torch _foreach composition": self.step}


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def measure(graphs, rounds, replays):
    times = {k: [] for k in graphs}
    names = list(graphs)
    for r in range(rounds):
        for k in (names if r % 2 == 0 else names[::-1]):             # both orders
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(replays):
                graphs[k].replay()
            stop.record()
            stop.synchronize()
            times[k].append(start.elapsed_time(stop) * 1e3 / replays)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--replays", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tf_update: no GPU (a timing needs one)")
    real = real_list()
    total = sum(n for n, _ in real)
    out = {"total_elements": total, "bytes_per_buffer": 4 * total, "rounds": args.rounds, "replays": args.replays, "lists": {}}
    for name, variables in (("real (%d variables)" % len(real), real), ("equal 64K segments (%d)" % len(equal_list(total)), equal_list(total))):
        fused, foreach = Fused(variables), Foreach(variables)
        fns = dict(fused.variants(), **foreach.variants())
        graphs = {k: capture(fn) for k, fn in fns.items()}
        for g in graphs.values():                                    # warm-up replays of every variant
            for _ in range(5):
                g.replay()
        torch.cuda.synchronize()
        times = measure(graphs, args.rounds, args.replays)
        res = {}
        for k, ts in times.items():
            q1, med, q3 = np.percentile(ts, [25, 50, 75])
            res[k] = {"median_us": round(float(med), 2), "min_us": round(float(min(ts)), 2), "iqr_us": round(float(q3 - q1), 2)}
        med = res["fused clip_and_step"]["median_us"]
        res["fused clip_and_step"]["fraction_of_8TBs_at_28B_per_element"] = round(28 * total / (med * 1e-6) / PEAK, 3)
        res["ratio_foreach_over_fused"] = round(res["torch _foreach composition"]["median_us"] / med, 3)
        res["variables"], res["chunks"] = len(variables), fused.opt.layout.n_chunks
        out["lists"][name] = res
        del graphs, fused, foreach
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
