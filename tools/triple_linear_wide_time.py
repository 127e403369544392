#!/usr/bin/env python3
"""The q / k / v projections of the wide attention stages, forward + backward, two formulations in one process:
    arm A  the batched library products this project used before (baddbmm; bmm(...).sum(0), bmm, sum(1)) on adjacent weights, once with
           torch.backends.cuda.preferred_blas_library("cublas") (rocBLAS: what bench.py sets) and once with the library torch picks by default (what a caller who
           sets nothing got);
    arm B  cbl_triple_linear_forward / _backward (csrc/skinny_linear.hip).
At (n, C) = (2560, 128), (640, 256), (160, 512) and their 4- and 8-scene row counts.  Every arm is a captured hipGraph; the arms are replayed in turn
(A, A-default, B, A, ...) `--repeats` times, `--reps` replays between two HIP events each; per arm the median and the spread (min, max) of the repeats.
python tools/triple_linear_wide_time.py -> one JSON line (us per forward + backward)."""
import argparse
import ctypes
import json
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from contrastboundary_amd import _lib  # noqa: E402

STAGES = [(2560, 128), (640, 256), (160, 512)]


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn(); fn(); fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        fn()
    return g, s


def replay_us(g, s, reps):
    with torch.cuda.stream(s):
        g.replay()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            g.replay()
        b.record()
        b.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def library_arm(x, W3, b3, g_qkv, keep):
    n, C = x.shape

    def fn():
        keep["qkv"] = torch.baddbmm(b3.unsqueeze(1), x.unsqueeze(0).expand(3, n, C), W3.transpose(1, 2))
        keep["g_x"] = torch.bmm(g_qkv, W3).sum(0)
        keep["g_W3"] = torch.bmm(g_qkv.transpose(1, 2), x.unsqueeze(0).expand(3, n, C))
        keep["g_b3"] = g_qkv.sum(1)
    return fn


def entries_arm(x, W3, b3, g_qkv, keep):
    n, C = x.shape
    L = _lib.lib()
    ws = torch.empty(L.cbl_triple_linear_workspace_bytes(ctypes.c_int(C)), dtype=torch.uint8, device=x.device)
    arr = lambda t: (ctypes.c_void_p * 3)(*[t[p].data_ptr() for p in range(3)])

    def fn():
        qkv, g_x, g_W3, g_b3 = torch.empty_like(g_qkv), torch.empty_like(x), torch.empty_like(W3), torch.empty_like(b3)
        st = _lib.stream_of(x)
        _lib.check(L.cbl_triple_linear_forward(ctypes.c_longlong(n), ctypes.c_int(C), _lib.ptr(x), arr(W3), arr(b3), arr(qkv), st), "forward")
        _lib.check(L.cbl_triple_linear_backward(ctypes.c_longlong(n), ctypes.c_int(C), _lib.ptr(x), arr(W3), arr(g_qkv), _lib.ptr(g_x), arr(g_W3), arr(g_b3),
                                                _lib.ptr(ws), ctypes.c_size_t(ws.numel()), st), "backward")
        keep.update(qkv=qkv, g_x=g_x, g_W3=g_W3, g_b3=g_b3)
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--once", action="store_true", help="one eager call of arm B per shape and nothing else (for a kernel trace)")
    args = ap.parse_args()
    default_lib = str(torch.backends.cuda.preferred_blas_library())
    out = {"device": torch.cuda.get_device_name(0), "unit": "us per forward + backward (hipGraph replay)", "default_blas_library": default_lib,
           "repeats": args.repeats, "replays_per_repeat": args.reps, "shapes": {}}
    torch.manual_seed(0)
    for n1, C in STAGES:
        for scenes in (1, 4, 8):
            n = n1 * scenes
            x = torch.randn(n, C, device="cuda")
            W3 = torch.randn(3, C, C, device="cuda") / C ** 0.5
            b3 = torch.randn(3, C, device="cuda")
            g_qkv = torch.randn(3, n, C, device="cuda")
            keeps = {k: {} for k in ("A_rocblas", "A_default", "B")}
            if args.once:
                entries_arm(x, W3, b3, g_qkv, keeps["B"])()
                torch.cuda.synchronize()
                continue
            torch.backends.cuda.preferred_blas_library("cublas")
            graphs = {"A_rocblas": capture(library_arm(x, W3, b3, g_qkv, keeps["A_rocblas"]))}
            torch.backends.cuda.preferred_blas_library(default_lib.rsplit(".", 1)[-1].lower())
            graphs["A_default"] = capture(library_arm(x, W3, b3, g_qkv, keeps["A_default"]))
            graphs["B"] = capture(entries_arm(x, W3, b3, g_qkv, keeps["B"]))
            ts = {k: [] for k in graphs}
            for _ in range(args.repeats):
                for k, (g, s) in graphs.items():
                    ts[k].append(replay_us(g, s, args.reps))
            r = {"rows": n, "C": C}
            for k, v in ts.items():
                r[k] = {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
            ref = keeps["A_rocblas"]
            r["B_vs_A_max_rel_diff"] = max(float((keeps["B"][k] - ref[k]).abs().max() / ref[k].abs().max()) for k in ("qkv", "g_x", "g_W3", "g_b3"))
            out["shapes"]["%dx%d" % (n, C)] = r
    if not args.once:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
