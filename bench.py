#!/usr/bin/env python3
"""bench.py — points/sec through the KNN + group + local-aggregation + CBL block on S3DIS-shaped synthetic scenes.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--points 40960] [--channels 64] [--k 16] [--forward-only] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A plain run sets the step up, runs W warm-up steps, times exactly K steps in one region and prints the headline (`metric`, `value`, `unit`,
`higher_is_better`, `dtype`, `ms_per_step`, ...).  `--dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy (same arguments,
same inputs: two builds can be compared output for output).  `--full` adds the median of three timed regions as the headline and everything the
line carries beside it (below).

One "step" = one pass of the hot path (contrastboundary_amd/hotpath.py: search, gather, KPConv, CBL head forward + backward and — BASELINE
config C2 "forward/backward" — the block's backward legs) over one scene whose inputs are already resident in HBM.  Scenes are independent,
so N ranks run N scene replicas with no data-path collective (weak scaling).  `--gpus N` without a torchrun environment
re-executes this file under torch.distributed.run with N ranks (one per device; fewer than N devices is an error); the printed `n_gpus` is the
number of ranks that joined the process group.  Every timed step is the same thing: the step's hipGraphs replayed, consecutive steps
software-pipelined (hotpath.Pipeline: the search of step i+1 beside the gather / KPConv / backward kernels of step i; `--no-pipeline`: one
graph per step, every step on its own).  The timed region is bracketed by barrier + synchronize (the whole device) and the MAX over ranks is
used.  Rank 0 prints ONE JSON line with the driver's fields, and with `--full`
  `roofline`      the HBM-bound neighbour gather: algorithmic bytes / HIP-event duration of its launch alone (back-to-back launches behind a
                  filler kernel, events on the launch stream), with the K4 gather and the KPConv kernel beside it, the in-order per-stage
                  times, PMC traffic from profiles/ if it belongs to this kernel set;
  `forward_only`  the forward block + CBL head alone (round 1's step), timed the same way;
  `grad_allreduce` (N > 1) the same K steps with one flat 31.2 MB fp32 all-reduce per step over RCCL beside the compute — what DDP adds to
                  data-parallel training of the reference's network (pytorch/tool/train.py:141,181-185; 7,800,497 parameters);
  `cpu_baseline`  (N = 1, rank 0) tests/cpu_baseline.py: the reference's own CPU KNN (oracle/_ref) and the CPU oracles on the host cores.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.29 TB/s measured copy)
FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: f32 matrix = f32 vector peak
GRAD_ALLREDUCE_FLOATS = 7800497   # parameters of the reference's PointTransformerSeg + heads: 31.2 MB fp32
PMC_FILE = os.path.join(ROOT, "profiles", "r06_pmc_traffic.json")     # collected by tools/gpu_r06_final.sh; its _meta.commit names the kernel set
PMC_MIX_FILE = os.path.join(ROOT, "profiles", "r06_pmc_instruction_mix.json")   # same script: SQ_* counters per kernel of the same command (separate --pmc passes)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", type=int, default=None, help="points per scene (default: 40960 for the block, 200000 for the ConvNet workload)")
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--workload", choices=("block", "convnet", "stage_shapes"), default="block",
                    help="block: BASELINE's headline (KNN + group + KPConv + CBL, N=40960); convnet: config C5 / the per-scene work of C3 "
                         "(radius + grid pyramid of a 200000-point cloud, AdaptiveWeight forward + backward on its 5 layers, TF-side CBL); stage_shapes: "
                         "gather / attention layer / FPS at the Point Transformer's five REAL stage shapes (SURVEY 8 caveat), a measurement, no step")
    ap.add_argument("--block", choices=("kpconv", "pt"), default="kpconv",
                    help="local aggregation of the block: kpconv = BASELINE's headline (KNN + group + KPConv + CBL); pt = the Point Transformer's vector "
                         "attention layer in its place (BASELINE.md: a1 + a3 + a4 + a8, pytorch/model/blocks.py:31-44)")
    ap.add_argument("--forward-only", action="store_true", help="headline = forward block + CBL head only (round 1's step)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-overlap", action="store_true", help="all stages in order on one stream")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="every step on its own (one hipGraph per step) instead of consecutive steps software-pipelined: the search of step i+1 beside the rest of step i")
    ap.add_argument("--no-graph", action="store_true", help="issue every step eagerly from Python instead of replaying its hipGraph")
    ap.add_argument("--no-nested", action="store_true", help="every neighbour search on its own (no derivation of K=16 from the K=36 search of the same points)")
    ap.add_argument("--no-allreduce", action="store_true", help="skip the gradient all-reduce leg of a multi-rank run")
    ap.add_argument("--no-extra", action="store_true", help="headline only: no forward_only / stage / all-reduce legs (profiling runs)")
    ap.add_argument("--no-gather-200k", action="store_true", help="skip the HBM-certain gather measurement (N = 200 000: 857 MB per launch) of the roofline object")
    ap.add_argument("--no-legs", action="store_true",
                    help="default line only: skip the `pt_block` (config C4) and `convnet` (configs C5 / C3 per scene) legs the 1-GPU --full run appends")
    ap.add_argument("--allreduce-floats", type=int, default=GRAD_ALLREDUCE_FLOATS)
    ap.add_argument("--allreduce-single", action="store_true",
                    help="tests: run the gradient all-reduce leg over a ONE-rank RCCL group (exercises the RCCL path on a 1-GPU box; not a scaling number)")
    ap.add_argument("--host-dry-run", action="store_true",
                    help="CPU-only run of the launcher / process-group / timing / all-reduce logic over gloo (tests; not a measurement)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: three timed regions (median), roofline and per-stage times, forward_only / no_pipeline / all-reduce "
                         "steps, cpu_baseline and the legs of the other workloads.  Without it a run sets up, warms up, times exactly --steps steps once "
                         "and prints the headline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32 / float64; integer outputs as float64, "
                         "the order-free K=36 rows sorted; at most 60 MB: past that, the largest per-point outputs keep one seeded sample of rows, DIR/rows.npy)")
    args = ap.parse_args(argv)
    if args.points is None:
        args.points = 200000 if args.workload == "convnet" else 40960
    return args


# ------------------------------------------------------------------------------------------------ launcher
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def spawn(args, argv):
    """`--gpus N` outside a torchrun environment: re-execute under torch.distributed.run, one rank per GPU (what the driver does itself)"""
    if not args.host_dry_run:
        have = torch.cuda.device_count()
        if have < args.gpus:
            sys.stderr.write("bench.py: --gpus %d but only %d device(s) visible; refusing to report a smaller run as n_gpus=%d\n" % (args.gpus, have, args.gpus))
            return 2
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")               # dmabuf IPC (RCCL / CUDA-tensor sharing across processes)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    return subprocess.call(cmd, env=env)


def timed_region(step, steps, warmup, sync, D):
    """W untimed steps, then EXACTLY K steps between barrier + synchronize on both sides; -> max over ranks of the wall time
    (sync = torch.cuda.synchronize: the whole device, whatever streams the steps run on)"""
    for _ in range(warmup):
        step()
    sync()
    D.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    timed_region.issue_s = time.perf_counter() - t0                  # host time to ISSUE the K steps (diagnostic: equal to the wall time = host bound)
    sync()
    mine = time.perf_counter() - t0                                  # this rank's own K steps, before the closing barrier
    D.barrier()
    total = time.perf_counter() - t0
    timed_region.per_rank_ms = (D.reduce_scalar(mine, "min") / steps * 1e3, D.reduce_scalar(mine, "max") / steps * 1e3)
    return D.reduce_scalar(total, "max")


def timed_median(step, steps, warmup, sync, D, regions=3):
    """The headline's clock: `regions` timed regions of EXACTLY `steps` steps each, one after the other in this process (W warm-up steps in front of the first),
    every one bracketed by barrier + synchronize on both sides with the max over ranks — the value reported is the MEDIAN region's (20 steps of 0.3 ms are
    6 ms: one region is inside the box's noise, round-4 review item 8).  -> (median elapsed seconds, [ms per step of every region]); `timed_region.issue_s` /
    `.per_rank_ms` are left holding the median region's values."""
    runs = []
    for r in range(regions):
        e = timed_region(step, steps, warmup if r == 0 else 0, sync, D)
        runs.append((e, timed_region.issue_s, timed_region.per_rank_ms))
    mid = sorted(runs, key=lambda t: t[0])[len(runs) // 2]
    timed_region.issue_s, timed_region.per_rank_ms = mid[1], mid[2]
    return mid[0], [round(e / steps * 1e3, 5) for e, _, _ in runs]


def rank_spread(D):
    """{"rccl_ranks": ranks of the process group, "backend", "ms_per_step_min_rank" / "_max_rank": the fastest and the slowest rank's own time per step
    of the LAST timed region (before its closing barrier)} — the multi-GPU line's evidence that N processes took part and how evenly"""
    ranks, backend = D.group_ranks()
    lo, hi = getattr(timed_region, "per_rank_ms", (None, None))
    return {"rccl_ranks": ranks, "backend": backend, "ms_per_step_min_rank": lo, "ms_per_step_max_rank": hi}


class GradAllReduce:
    """one flat fp32 buffer all-reduced per step beside the compute, as DDP does with the network's gradients (train.py:181-185)"""

    def __init__(self, nfloats, device):
        import torch.distributed as dist
        self.dist = dist
        self.buf = torch.ones(nfloats, dtype=torch.float32, device=device)
        self.pending = []

    def start(self):
        self.pending.append(self.dist.all_reduce(self.buf, op=self.dist.ReduceOp.SUM, async_op=True))

    def finish(self):
        for w in self.pending:
            w.wait()                                                 # the current stream waits for the collective (no host block on a GPU)
            self.buf.mul_(1.0 / self.dist.get_world_size())          # keep the values bounded over many steps: average like DDP
        self.pending = []


def timed_headline(step, args, sync, D):
    """the headline's clock: exactly --steps timed steps in one region (timed_region); --full keeps three regions and reports the median one
    (timed_median).  -> (elapsed seconds, [ms per step of every region])"""
    if args.full:
        return timed_median(step, args.steps, args.warmup, sync, D)
    e = timed_region(step, args.steps, args.warmup, sync, D)
    return e, [round(e / args.steps * 1e3, 5)]


REGIONS_NOTE = {True: "three regions of --steps steps each, barrier + synchronize around every one; value / ms_per_step = the median region",
                False: "one region of exactly --steps steps, barrier + synchronize around it (--full: three regions, the median one)"}


# ------------------------------------------------------------------------------------------------ --dump-outputs
DUMP_CAP_BYTES = 60 * 10 ** 6
DUMP_KEYS = ("idx", "dist2", "grouped", "kpconv", "pt_out", "cbl_idx", "cbl_loss", "cbl_grad", "grad_feat_group", "grad_feat_kpconv",
             "grad_kernel_weights", "grad_feat_pt", "grad_params_pt")


def dump_outputs(state, n, out_dir, seed=0):
    """what one step of the block hands its caller (hotpath.stages / stages_pt state) as out_dir/<name>.npy: float outputs as float32, integer ones
    as float64 (exact), the K=36 rows of the order-free CBL search sorted (the set is the result, not its order).  If everything does not fit in
    DUMP_CAP_BYTES, the largest outputs whose first axis is the scene's n points keep one seeded sample of rows (out_dir/rows.npy), shared by
    all of them, and the others are written whole.  -> {name: shape}"""
    arrays = {}
    for key in DUMP_KEYS:
        v = state.get(key)
        if v is None:
            continue
        for i, t in enumerate(v) if isinstance(v, (tuple, list)) else [(None, v)]:
            a = t.detach().cpu().numpy()
            if key == "cbl_idx":
                a = np.sort(a, axis=1)
            arrays[key if i is None else "%s_%d" % (key, i)] = a.astype(np.float32 if np.issubdtype(a.dtype, np.floating) else np.float64)
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_CAP_BYTES:
        per_point = sorted((nm for nm, a in arrays.items() if a.ndim and a.shape[0] == n), key=lambda nm: arrays[nm].nbytes)
        sampled, whole = [], total
        while per_point and whole > DUMP_CAP_BYTES * 3 // 4:      # a quarter of the budget at least for the sampled rows
            sampled.append(per_point.pop())
            whole -= arrays[sampled[-1]].nbytes
        m = min(n, (DUMP_CAP_BYTES - whole) // (8 + sum(arrays[nm].nbytes // n for nm in sampled)))
        rows = np.sort(np.random.default_rng(seed).choice(n, m, replace=False))
        for nm in sampled:
            arrays[nm] = arrays[nm][rows]
        arrays["rows"] = rows.astype(np.float64)
    assert sum(a.nbytes for a in arrays.values()) <= DUMP_CAP_BYTES
    os.makedirs(out_dir, exist_ok=True)
    for nm, a in arrays.items():
        np.save(os.path.join(out_dir, nm + ".npy"), a)
    return {nm: list(a.shape) for nm, a in arrays.items()}


# ------------------------------------------------------------------------------------------------ host dry run (gloo, CPU): tests only
def host_dry_run(args, D, world, rank):
    """the N > 1 logic of this file without a GPU: rendezvous, world-size check, barrier-bracketed timing, max over ranks, the all-reduce
    leg, one JSON line from rank 0.  The 'step' is a fixed sleep: nothing here is a measurement."""
    D.init("gloo")
    import torch.distributed as dist
    assert (dist.get_world_size() if dist.is_initialized() else 1) == args.gpus, "process group size != --gpus"
    n = args.points

    def step():
        time.sleep(0.002)
    elapsed = timed_region(step, args.steps, args.warmup, lambda: None, D)
    out = {"ranks": rank_spread(D), "metric": "host dry run (NOT a measurement)", "value": n * args.steps * world / elapsed, "unit": "points/s", "n_gpus": world, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "f32", "data": "none (host dry run over gloo)",
           "config": {"workload": "sleep standing in for %s" % ("the ConvNet scene step" if args.workload == "convnet" else "the %s block" % args.block),
                      "parallelism": "replicas x%d" % world}}
    if world > 1 and not args.no_allreduce:
        ar = GradAllReduce(args.allreduce_floats, "cpu")

        def step_ar():
            ar.start(); step(); ar.finish()
        e2 = timed_region(step_ar, args.steps, args.warmup, lambda: None, D)
        out["grad_allreduce"] = {"value": n * args.steps * world / e2, "ms_per_step": e2 / args.steps * 1e3, "bytes": 4 * args.allreduce_floats,
                                 "checksum": float(ar.buf[0])}
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist.is_initialized():
        dist.destroy_process_group()
    return 0


# ------------------------------------------------------------------------------------------------ the step
# measured in one gpurun call each (profiles/r06_pair_tables_ab.txt), three runs per arm: Point Transformer block pipelined 0.486 -> 0.477 ms, one step at a time
# 0.624 -> 0.600; KPConv block pipelined 0.280 -> 0.284 ("pair_split"; the pair build on the search stream: 0.349), one step at a time unchanged (its block table
# is built on a stream of its own beside the forward either way)
PAIR_TABLES_DEFAULT = {"pt": "1", "kpconv": "0"}


def pair_layout_forced(step):
    """CBL_PIPELINE_LAYOUT only applies where it fits how the step's stages build their tables (a forward-only step builds no pair: its layouts are the plain ones)"""
    env = os.environ.get("CBL_PIPELINE_LAYOUT")
    return bool(env) and env.startswith("pair_") != step.pair_tables


class Step:
    """the hot path over one resident scene as bench.py runs it: schedule + its hipGraph(s).
    pipeline: consecutive steps software-pipelined over four streams, one linear hipGraph per chain (hotpath.Pipeline: the search of step i+1
    beside the forward kernels of step i and the backward kernels of step i-1); steps rotate through the pipeline's output slots (self.states)."""

    def __init__(self, scene, k, backward, args, overlap=True, pipeline=False, pair_tables=None):
        from contrastboundary_amd import hotpath
        self.block = getattr(args, "block", "kpconv")
        # the two transposed tables of the step's one geometry (K = 36 for the CBL head, K = 16 for the block) by one set of launches (cbl_neighbor_transpose_pair);
        # CBL_PAIR_TABLES=0 (or a CBL_PIPELINE_LAYOUT that is not a "pair_" one): one after the other, each on the stream of its consumer (the round-5 step)
        env_layout = os.environ.get("CBL_PIPELINE_LAYOUT")
        if pair_tables is None:
            pair_tables = env_layout.startswith("pair_") if env_layout else os.environ.get("CBL_PAIR_TABLES", PAIR_TABLES_DEFAULT[self.block]) != "0"
        self.pair_tables = bool(backward) and bool(pair_tables)
        self.stages = (hotpath.stages_pt if self.block == "pt" else hotpath.stages)(scene, k, backward, pair_tables=self.pair_tables)
        self.names = [st[0] for st in self.stages]
        self.hints = () if args.no_nested else hotpath.search_hints(scene)
        self.sched = hotpath.Schedule(self.stages, overlap=overlap, hints=self.hints, aux_tables=getattr(args, "block", "kpconv") != "pt", pair_tables=self.pair_tables)
        self.pipeline = bool(pipeline and overlap and self.hints)
        self.pipe = None
        self.states = [{}]
        self.graph, self.note = None, "eager"

    @property
    def state(self):
        return self.states[-1]

    def last_state(self):
        """the outputs of the step issued last (the pipeline's steps rotate through its slots)"""
        if self.pipe is not None:
            return self.pipe.states[(self.pipe.count - 1) % self.pipe.SLOTS]
        return self.states[0]

    def eager(self, events=None):
        self.sched.run(self.states[0], events)

    def capture(self):
        """the step issues 30-40 launches from Python, as many us of host time as the device needs: captured once (same kernels, same
        buffers, same schedule) it is replayed with ~15 us of host time.  Raises if the capture fails (bench.py then stays eager)."""
        # what the eager runs left behind goes first: autograd keeps a parameter's gradient accumulator (and the stream it was created on — here the
        # default stream) for as long as a graph of an earlier step is referenced, and a capture of the backward pass that meets such a node
        # synchronises with the default stream (a crash on ROCm 7.2).  The Point Transformer block's layer has parameters; KPConv's leaves are per step.
        import gc
        self.states = [{}]
        gc.collect()
        if self.pipeline:
            from contrastboundary_amd import hotpath
            # KPConv block: the backward on a stream of its own, the CBL chain's table first, three slots; Point Transformer block (its backward chain is 0.46 of
            # the 0.55 ms): consecutive steps' backward chains on two streams in turn, four slots — all measured against the other layouts in one call (hotpath.Pipeline)
            default_layout = ("pair_alt_bwd" if self.block == "pt" else "pair_split") if self.pair_tables else ("alt_bwd" if self.block == "pt" else "split_t36_first")
            pipe = hotpath.Pipeline(self.sched, layout=(os.environ.get("CBL_PIPELINE_LAYOUT") if not pair_layout_forced(self) else None) or default_layout,
                                    slots=os.environ.get("CBL_PIPELINE_SLOTS") or (4 if self.block == "pt" else 3))
            pipe.capture()
            self.pipe, self.states = pipe, pipe.states
            self.note = "hipGraph replay (torch.cuda.CUDAGraph over the C-ABI launches), " + pipe.describe()
            return
        cap = torch.cuda.Stream()
        cap.wait_stream(torch.cuda.current_stream())
        gstate = {}
        with torch.cuda.stream(cap):
            for _ in range(3):
                self.sched.run(gstate, None)
        torch.cuda.current_stream().wait_stream(cap)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):     # other threads (the RCCL watchdog of a multi-rank run) may call HIP
            self.sched.run(gstate, None)
        g.replay()
        torch.cuda.synchronize()
        self.graph, self.states = g, [gstate]
        self.note = "hipGraph replay (torch.cuda.CUDAGraph over the C-ABI launches)"

    def __call__(self):
        if self.pipe is not None:
            self.pipe.step()
        elif self.graph is not None:
            self.graph.replay()
        else:
            self.sched.run(self.states[0], None)

    def join(self):
        """the current stream waits for every step issued so far (the pipeline runs on streams of its own)"""
        if self.pipe is not None:
            self.pipe.join()


def settle(step, seconds=0.5):
    """not part of the W warm-up steps: first touches of the library, workspaces and code objects, clock ramp of a cold device"""
    t = time.perf_counter()
    while time.perf_counter() - t < seconds:
        step.eager()
        torch.cuda.synchronize()


def make_step(scene, k, backward, args, overlap, pipeline=False):
    st = Step(scene, k, backward, args, overlap=overlap, pipeline=pipeline and not args.no_graph)
    settle(st)
    if not args.no_graph:
        try:
            st.capture()
        except Exception as e:                                       # noqa: BLE001 - any capture problem: stay eager, and say so
            st.graph, st.note = None, "eager (graph capture failed: %s: %s)" % (type(e).__name__, str(e)[:80])
            torch.cuda.synchronize()
    return st


def checked_pipeline_step(scene, k, backward, args, overlap, pipeline):
    """make_step, plus a check of what the stream probe (hotpath.concurrent_streams) promised: a software pipeline whose streams share hardware queues runs
    its segments in order and costs what one step at a time costs (seen once in ~30 processes: 0.43 instead of 0.28 ms per step, every timed region alike).
    The pipelined step is held against the same step issued one at a time over a few untimed steps (no barrier: every rank decides for itself); if it
    gains less than 8 %, the pipeline is rebuilt on freshly probed streams, at most twice.  -> (step, {"pipelined_ms", "one_at_a_time_ms", "rebuilt"})"""
    step = make_step(scene, k, backward, args, overlap=overlap, pipeline=pipeline)
    if step.pipe is None:
        return step, None

    def local_ms(st, n=20):
        for _ in range(5):
            st()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            st()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n * 1e3
    ref = make_step(scene, k, backward, args, overlap=True, pipeline=False)
    one = local_ms(ref)
    del ref
    rebuilt, got = 0, local_ms(step)
    force = bool(os.environ.get("CBL_PIPELINE_CHECK_FORCE"))          # exercise the rebuild once (tools / tests)
    while (got > 0.92 * one or (force and rebuilt == 0)) and rebuilt < 2:
        del step
        torch.cuda.synchronize()
        step = make_step(scene, k, backward, args, overlap=overlap, pipeline=pipeline)
        rebuilt, got = rebuilt + 1, local_ms(step)
    return step, {"pipelined_ms": round(got, 4), "one_at_a_time_ms": round(one, 4), "rebuilt": rebuilt,
                  "note": "untimed steps before the timed regions: a pipeline that gains < 8 % over one step at a time is rebuilt on freshly probed streams"}


def stage_times(scene, k, backward, args, reps=8):
    """per-stage device time of the step IN ORDER on one stream -> (step, ms per stage, how).  Round 6: differences of PREFIX graphs — the stages 0..i of the
    in-order step captured as one hipGraph per i, every graph replayed back to back between two HIP events; stage i = T(0..i) - T(0..i-1).  No host time can
    enter (a replay is one launch; the eager harness below read 0.42 ms for the attention layer's backward whose graph takes 0.27: its ~40 launches out-ran the
    filler on a slow host), the per-replay overhead of a graph cancels in the difference, and every stage runs behind the stages it follows in the step (same
    cache state).  Falls back to the eager harness (events around eagerly issued stages behind filler kernels) if a capture fails."""
    try:
        return stage_times_prefix_graphs(scene, k, backward, args, reps)
    except Exception as e:                                           # noqa: BLE001 - any capture problem: the eager harness, and say so
        torch.cuda.synchronize()
        st, ms, how = stage_times_eager(scene, k, backward, args, reps)
        return st, ms, how + " (prefix-graph harness failed: %s: %s)" % (type(e).__name__, str(e)[:80])


def stage_times_prefix_graphs(scene, k, backward, args, reps=8):
    import gc
    from contrastboundary_amd import hotpath
    st = Step(scene, k, backward, args, overlap=False)
    settle(st, 0.2)
    gc.collect()
    cap = torch.cuda.Stream()
    graphs, state = [], None
    for i in range(len(st.stages)):
        sched = hotpath.Schedule(st.stages[:i + 1], overlap=False, hints=st.hints, pair_tables=st.pair_tables)
        gstate = {}
        cap.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(cap):
            sched.run(gstate, None)                                  # once eagerly: workspaces of this stream, code objects
        torch.cuda.current_stream().wait_stream(cap)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=cap, capture_error_mode="thread_local"):
            sched.run(gstate, None)
        graphs.append(g); state = gstate
    inner = 5

    def timed(g):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(cap):
            g.replay()
            a.record()
            for _ in range(inner):
                g.replay()
            b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / inner
    for g in graphs:
        g.replay()
    torch.cuda.synchronize()
    samples = [[timed(g) for g in graphs] for _ in range(max(3, reps // 2))]
    T = np.median(np.asarray(samples), axis=0)
    ms = [float(T[0])] + [float(max(T[i] - T[i - 1], 0.0)) for i in range(1, len(T))]
    st.states = [state]                                               # the full step's outputs (the last prefix), for the callers that check them
    how = ("differences of prefix graphs: stages 0..i of the in-order step as one hipGraph per i, %d back-to-back replays between two HIP events, median of %d rounds; "
           "stage i = T(0..i) - T(0..i-1) (device time with a graph's launch gaps, no host issue time; the first stage also carries a replay's fixed cost)"
           % (inner, len(samples)))
    return st, ms, how


def stage_times_eager(scene, k, backward, args, reps=8):
    """the round-5 harness: HIP events on the launch stream around every stage of eagerly issued in-order steps.  The steps are issued behind filler kernels
    sized from the host's own issue time of one step (1.5 x), so the host is a whole step ahead of the device and an interval holds the stage's kernels and
    their launch gaps, not the host — as long as the host out-runs the device inside the step too."""
    st = Step(scene, k, backward, args, overlap=False)
    settle(st, 0.2)
    filler = torch.empty(1 << 31, dtype=torch.uint8, device="cuda")
    # how long the host needs to issue one step, and how long one fill of the filler keeps the device busy: the step is issued behind enough fills that the
    # device is still in them when the host is done (round 5: a fixed 0.6 ms was shorter than a slow host's issue time, and the late stages read host time)
    torch.cuda.synchronize()
    t0 = time.perf_counter(); st.eager(); host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); filler.fill_(0); b.record(); torch.cuda.synchronize()
    fill_ms = max(a.elapsed_time(b), 0.05)
    fills = int(min(64, max(2, np.ceil(1.5 * host_ms / fill_ms))))
    samples = []
    for _ in range(reps + 2):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in st.stages]
        for f in range(fills):
            filler.fill_(f & 1)
        st.eager(ev)
        torch.cuda.synchronize()
        samples.append([a.elapsed_time(b) for a, b in ev])
    del filler
    how = ("HIP events on the launch stream around every stage of eagerly issued in-order steps, each issued behind %d fills of a 2 GiB buffer (%.2f ms of device work "
           "for %.2f ms of host issue time per step: the host stays ahead of the device), median of %d right after the timed region" % (fills, fills * fill_ms, host_ms, reps))
    return st, [float(v) for v in np.median(np.asarray(samples[2:]), axis=0)], how


def kernel_times(scene, k, backward, reps=10):
    """launch duration of the roofline kernels, each ALONE: `reps` back-to-back launches of one stage behind a filler kernel, two HIP events
    on the launch stream around the whole run (an event pair around a single launch costs about as much device time as a small kernel:
    `stage_ms` carries that, these do not).  Same tensors, same processing order and same transposed table as the step."""
    from contrastboundary_amd import hotpath, local_aggregation, pointops
    n, c = scene.n, scene.c
    out = {}
    filler = torch.empty(1 << 32, dtype=torch.uint8, device="cuda")

    def timed(fn):
        # the outputs of the last three launches stay referenced: consecutive launches write DIFFERENT buffers (the caching allocator would
        # otherwise hand every launch the buffer the previous one just freed, and a 190 MB output re-written in place sits in the 256 MB Infinity Cache)
        ring = [fn(), fn(), fn()]                                   # all three buffers exist before anything is timed (round 6: one run in ~20 read 940 us for the
        torch.cuda.synchronize()                                     # 39 us gather — the third buffer's first allocation, a device malloc, inside the timed region)
        rounds = []
        for _ in range(3):                                           # ... and one glitch does not decide the figure: the median of three rounds
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            filler.fill_(0); filler.fill_(1)                         # ~1.2 ms: the host enqueues all `reps` launches meanwhile
            a.record()
            for r in range(reps):
                ring[r % 3] = None                                   # freed first: the allocator hands the same three blocks round
                ring[r % 3] = fn()
            b.record()
            torch.cuda.synchronize()
            rounds.append(a.elapsed_time(b) / reps * 1e3)            # us
        return sorted(rounds)[1]
    with pointops.neighbor_cache() as nc:
        for xyz, nsample, algo in hotpath.search_hints(scene):
            nc.hint(xyz, nsample, algo)
        idx, _ = pointops.knnquery_raw(k, scene.xyz, scene.xyz, scene.offset, scene.offset)
        out["queryandgroup"] = timed(lambda: pointops.queryandgroup(k, scene.xyz, scene.xyz, scene.feat, idx, scene.offset, scene.offset, use_xyz=True))
        out["kpconv_fwd"] = timed(lambda: local_aggregation.kpconv(scene.xyz, scene.xyz, idx, scene.feat, scene.kernel_points, scene.kernel_weights, 0.12))
        if backward:
            up = scene.upstream(k)
            pointops.neighbor_transpose(idx, n)
            out["queryandgroup_bwd"] = timed(lambda: pointops._scatter_rows(up["grad_grouped"], idx, n, 3, c))
    del filler
    return out


def search_roofline(scene, k, stage_ms, nested):
    """The step's longest stage is the neighbour search, and its bound is neither HBM nor the matrix cores (compulsory bytes 6 MB): a cell-list
    search is priced in PAIRS VISITED (candidate supports whose distance a query evaluates) against the n_cloud pairs per query of the brute-force kernel it
    replaces (knnquery_cuda_kernel.cu:65-111), and in the share of the device's vector-issue slots its kernel fills (PMC, profiles/)."""
    from contrastboundary_amd import hotpath, pointops
    ks = hotpath.CBL_NSAMPLE if nested else k                       # the search that actually runs (the K = 16 rows are derived from it)
    cnt = pointops.knn_block_candidates(ks, scene.xyz, scene.offset, "set")
    pairs = int(cnt.to(torch.int64).sum().item())
    ends = scene.offset.cpu().tolist()
    lens = [e - s for s, e in zip([0] + ends[:-1], ends)]
    brute = float(sum(l * l for l in lens))
    out = {"kernel": "knn_grid_wave_kernel<true, false> (K = %d, one wave per query: select-then-sort over the 27-cell block) behind the 6-launch grid build; "
                     "tie replay knn_replay_kernel" % ks,
           "stage": "knnquery_k%d" % k, "stage_ms": round(stage_ms, 4), "bound": "vector issue (VALU)", "nsample": ks,
           "pairs_visited": pairs, "pairs_per_query": round(pairs / scene.n, 1), "pairs_per_query_min_max": [int(cnt.min().item()), int(cnt.max().item())],
           "brute_force_pairs": brute, "pairs_vs_brute_force": pairs / brute,
           "pairs_per_s": pairs / (stage_ms * 1e-3), "candidate_read_GBps": 16.0 * pairs / (stage_ms * 1e-3) / 1e9,
           "note": "pairs visited = candidate supports in the 27-cell block of every query (cbl_knn_grid_block_candidates, recomputed from the grid the search built: "
                   "what its first round evaluates; a further shell is taken by well under 1 % of the queries); 16 B (float4) read per candidate from the "
                   "cell-sorted copy, L2-resident at this size — the kernel is bound by its vector instructions, not by those reads"}
    if os.path.exists(PMC_MIX_FILE) and (scene.n, scene.c, k) == (40960, 64, 16):
        mix = json.load(open(PMC_MIX_FILE))
        for name, v in mix.items():
            if name.startswith("knn_grid_wave_kernel") and isinstance(v, dict):
                out["valu_issue_fraction"] = v.get("valu_issue_utilisation")
                out["valu_instructions_per_launch"] = v.get("SQ_INSTS_VALU")
                out["valu_instructions_per_pair"] = (v.get("SQ_INSTS_VALU") or 0) * 64.0 / max(pairs, 1)    # lane-instructions per candidate pair
                out["kernel_us_under_counters"] = v.get("duration_us_at_2.4GHz")
                out["pmc_source"] = "%s (rocprofv3 --kernel-trace --pmc, separate passes; commit %s)" % (os.path.relpath(PMC_MIX_FILE, ROOT), mix.get("_meta", {}).get("commit", "?"))
                break
    return out


def gather_200k(n=200000, c=64, k=16, reps=10):
    """The gather at a size that is HBM for certain: S-room scaled to n = 200 000 points (same density), K = 16, C = 64 — output 4 n K (3 + C)
    = 857 MB per launch, past the 256 MiB Infinity Cache, consecutive launches alternating between three output buffers.  Returns the roofline
    entry: achieved = SURVEY 8(d) a3 bytes / HIP-event duration per launch, beside a fill of the same size measured the same way."""
    from contrastboundary_amd import hotpath, pointops
    scene = hotpath.Scene.synthetic(n, c, seed=7, b=1)
    with pointops.neighbor_cache():
        idx, _ = pointops.knnquery_raw(k, scene.xyz, scene.xyz, scene.offset, scene.offset)
        fn = lambda: pointops.queryandgroup(k, scene.xyz, scene.xyz, scene.feat, idx, scene.offset, scene.offset, use_xyz=True)
        ring = [fn(), fn(), fn()]
        torch.cuda.synchronize()

        def run(f):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for r in range(reps):
                f(r)
            b.record(); torch.cuda.synchronize()
            return a.elapsed_time(b) / reps * 1e3

        def gather(r):
            ring[r % 3] = None
            ring[r % 3] = fn()
        us = run(gather)
        fills = [torch.empty_like(ring[0]) for _ in range(3)]        # a fill of the same size, measured the same way (three buffers in rotation)
        for f in fills:
            f.fill_(0.0)
        torch.cuda.synchronize()
        us_fill = run(lambda r: fills[r % 3].fill_(1.0))
        del fills
    nbytes = 4 * n * k + 12 * n + 12 * n + 4 * n * c + 4 * n * k * (3 + c)
    out_bytes = 4 * n * k * (3 + c)
    pmc = {}
    if os.path.exists(PMC_FILE):
        pmc = json.load(open(PMC_FILE)).get("gather_200k", {})
    traffic = pmc.get("hbm_bytes_per_launch")
    del ring
    torch.cuda.empty_cache()
    return {"kernel": MAIN_KERNEL["queryandgroup"], "workload": "S-room scaled to N=%d (same density), K=%d, C=%d: %d MB per launch, three output buffers in rotation" % (n, k, c, nbytes // 1000000),
            "bound": "hbm", "achieved": nbytes / (us * 1e-6) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": nbytes / (us * 1e-6) / 1e9 / HBM_PEAK_GBS,
            "bytes_per_launch": nbytes, "launch_us": round(us, 2), "traffic": traffic,
            "traffic_over_bytes": (round(traffic / nbytes, 3) if traffic else None),
            "fill_same_size_GBps": round(out_bytes / (us_fill * 1e-6) / 1e9, 1), "frac_of_fill": round((nbytes / us) / (out_bytes / us_fill), 3),
            "note": "past the Infinity Cache (256 MiB): FETCH_SIZE / WRITE_SIZE of this launch are HBM traffic; `traffic` from %s when collected" % os.path.relpath(PMC_FILE, ROOT)}


MAIN_KERNEL = {
    "knnquery_k16": "grid build + knn_grid_wave_kernel (the K=36 search of the same points, which also writes the K=16 rows) + knn_replay_kernel for the tied rows",
    "queryandgroup": "query_group_lds_pipe<16, 16> (persistent waves, whole points as aligned pieces through LDS, next rows requested before the stores, cell-order schedule)",
    "kpconv_fwd": "kpconv_fwd_c64_kernel (v_mfma_f32_16x16x4_f32; branch-free, rows prefetched one point ahead)",
    "cbl_knnquery_k36": "cache hit on the wide search",
    "cbl_neighbor_transpose": "nt_prep / nt_count / nt_bin / nt_finish (transposed K=36 table)",
    "cbl_mining_loss_fwd": "contrast_pairs_kernel<8,5,true> + contrast_finalize_kernel",
    "cbl_mining_loss_bwd": "contrast_gather_kernel<8>",
    "neighbor_transpose_k16": "nt_prep / nt_count / nt_bin / nt_finish (transposed K=16 table)",
    "queryandgroup_bwd": "grouping_bwd_csr_rows_kernel (K4 as a gather)",
    "kpconv_bwd": "kpconv_bwd_csr_kernel<true,true,false> (S = W^T G over the transposed table, v_mfma_f32_16x16x4_f32) + kpconv_gkw_reduce_kernel",
}
PMC_KERNEL = {"queryandgroup": "query_group_lds_pipe<16, 16>", "kpconv_fwd": "kpconv_fwd_c64_kernel<false, true, true>", "cbl_mining_loss_fwd": "contrast_pairs_kernel<8, 5, true>",
              "cbl_mining_loss_bwd": "contrast_gather_kernel<8>", "queryandgroup_bwd": "grouping_bwd_csr_rows_kernel", "kpconv_bwd": "kpconv_bwd_csr_kernel<true, true, false>"}


def run_gpu(args, D, world, rank, local):
    torch.cuda.set_device(local)
    D.init("nccl" if world > 1 else None)                           # "nccl" is RCCL on ROCm
    if world == 1 and args.allreduce_single:
        import torch.distributed as dist
        if not dist.is_initialized():
            dist.init_process_group(backend="nccl", init_method="tcp://127.0.0.1:%d" % _free_port(), rank=0, world_size=1)
    if world > 1:
        import torch.distributed as dist
        assert dist.get_world_size() == args.gpus, "RCCL process group has %d ranks, --gpus says %d" % (dist.get_world_size(), args.gpus)
    from contrastboundary_amd import hotpath
    n, c, k = args.points, args.channels, args.k
    backward = not args.forward_only
    scene = hotpath.Scene.synthetic(n, c, seed=rank, b=1)            # every rank its own scene (weak scaling)
    pipeline = not (args.no_pipeline or args.no_overlap or args.no_nested or args.no_graph)
    step, pipe_check = checked_pipeline_step(scene, k, backward, args, overlap=not args.no_overlap, pipeline=pipeline)
    sync = torch.cuda.synchronize

    elapsed, regions = timed_headline(step, args, sync, D)
    spread = rank_spread(D)
    out = {
        "ranks": spread, "pipeline_check": pipe_check, "timed_regions_ms_per_step": regions, "timed_regions_note": REGIONS_NOTE[args.full],
        "metric": "points/sec through KNN+group+KPConv+CBL block, S3DIS N=40960 K=16",
        "value": n * args.steps * world / elapsed, "unit": "points/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "host_issue_ms_per_step": timed_region.issue_s / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": "S3DIS-shaped synthetic scene (S-room), N=%d, K=%d, C=%d, 1 scene per GPU per step, %s; stages: %s"
                   % (n, k, c, "forward + backward of the block" if backward else "forward block + CBL head", " -> ".join(step.names)),
                   "parallelism": "scene-per-GPU replicas x%d (no data-path collective)" % world,
                   "issue": step.note + ("; every timed step is the same replay" if (step.graph is not None or step.pipe is not None) else "; every timed step is issued from Python"),
                   "schedule": ("one search per geometry (the K=%d request runs the K=%d search the CBL head needs on the same points and is derived from it, tied "
                                "rows replayed; the later request is a cache hit, the cache is dropped at the end of every step); " % (k, hotpath.CBL_NSAMPLE)
                                if step.hints else "every search on its own; ") +
                               ("all stages in order on one stream" if args.no_overlap else "the CBL branch on a side stream beside the main branch") +
                               ("; consecutive steps software-pipelined: one stream carries the searches one after the other, everything behind a search runs "
                                "on three branch streams (forward | backward behind its table | CBL), so the search of step i+1 (grid build, wide search, tie "
                                "replay: mostly small latency-bound launches) runs beside the forward kernels of step i and the backward kernels of step i-1"
                                if step.pipe is not None else "")},
    }
    if args.dump_outputs and rank == 0:
        out["dumped_outputs"] = dump_outputs(step.last_state(), n, args.dump_outputs)
    if args.no_extra or not args.full:
        if rank == 0:
            print(json.dumps(out), flush=True)
        return finish(world)

    # ---- per-stage device times + roofline of the gather (in-order step, same process, right after the timed region)
    st_in, stage_ms, how = stage_times(scene, k, backward, args)
    names, stages = st_in.names, st_in.stages
    stage_bytes = [s[2] for s in stages]
    if st_in.hints:      # with the nested searches the first search stage does the work of both (the later request is a cache hit)
        first, later = names.index("knnquery_k%d" % k), names.index("cbl_knnquery_k%d" % hotpath.CBL_NSAMPLE)
        stage_bytes[first] += stage_bytes[later]
        stage_bytes[later] = 0
    gbps = lambda i: stage_bytes[i] / (stage_ms[i] * 1e-3) / 1e9 if stage_ms[i] > 0 else 0.0       # (a stage that launches nothing — a registry hit — measures 0)
    pmc = {}
    if os.path.exists(PMC_FILE) and (n, c, k) == (40960, 64, 16):
        pmc = json.load(open(PMC_FILE))
    traffic = lambda stage: pmc.get(PMC_KERNEL.get(stage, ""), {}).get("hbm_bytes_per_launch")
    gi = names.index("queryandgroup")
    dom = int(np.argmax(stage_ms))
    kus = kernel_times(scene, k, backward)                           # us per launch of the roofline kernels, each alone
    kgbps = lambda name: stages[names.index(name)][2] / (kus[name] * 1e-6) / 1e9
    roofline = {"kernel": MAIN_KERNEL["queryandgroup"], "stage": "queryandgroup", "bound": "hbm", "achieved": kgbps("queryandgroup"), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": kgbps("queryandgroup") / HBM_PEAK_GBS, "traffic": traffic("queryandgroup"), "bytes_per_launch": stages[gi][2],
                "launch_us": round(kus["queryandgroup"], 2),
                "traffic_source": ("PMC FETCH_SIZE (x2, gfx950 correction) + WRITE_SIZE per launch from %s, collected at commit %s (%s)"
                                   % (os.path.relpath(PMC_FILE, ROOT), pmc.get("_meta", {}).get("commit", "?"), pmc.get("_meta", {}).get("kernels", "this kernel set"))
                                   if traffic("queryandgroup") else "not measured for this kernel set (no %s)" % os.path.relpath(PMC_FILE, ROOT)),
                "note": "achieved = SURVEY 8(d) algorithmic bytes of the launch / its duration = HIP events on the launch stream around 10 back-to-back "
                        "launches of the kernel alone, issued behind a filler kernel, / 10 (same tensors, processing order and tables as the step; "
                        "rocprofv3 --kernel-trace --stats of this command: profiles/).  stage_ms: " + how,
                "longest_stage": {"stage": names[dom], "kernel": MAIN_KERNEL.get(names[dom], names[dom]), "ms": round(stage_ms[dom], 4),
                                  "algorithmic_GBps": round(gbps(dom), 1), "traffic": traffic(names[dom])},
                "stage_ms": {names[i]: round(stage_ms[i], 4) for i in range(len(stages))},
                "stage_sum_ms": round(float(sum(stage_ms)), 4),
                "stage_algorithmic_GBps": {names[i]: (round(gbps(i), 1) if stage_bytes[i] else None) for i in range(len(stages))}}
    roofline["search"] = search_roofline(scene, k, stage_ms[names.index("knnquery_k%d" % k)], bool(st_in.hints))
    if "queryandgroup_bwd" in names:
        bi = names.index("queryandgroup_bwd")
        roofline["scatter_k4"] = {"kernel": MAIN_KERNEL["queryandgroup_bwd"], "bound": "hbm", "achieved": kgbps("queryandgroup_bwd"), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                  "frac": kgbps("queryandgroup_bwd") / HBM_PEAK_GBS, "bytes_per_launch": stages[bi][2], "launch_us": round(kus["queryandgroup_bwd"], 2),
                                  "traffic": traffic("queryandgroup_bwd"),
                                  "note": "K4 (grouping_cuda_kernel.cu:16-25) as a gather over the transposed neighbour table: no atomics (round 1: 136 us, 17 % of HBM)"}
    ki = names.index("kpconv_fwd")
    tf = stages[ki][3] / (kus["kpconv_fwd"] * 1e-6) / 1e12
    roofline["mfma_kpconv"] = {"kernel": "kpconv_fwd_c64_kernel<false, true, true>", "bound": "mfma", "achieved": tf, "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                               "frac": tf / FP32_MFMA_PEAK_TFLOPS, "launch_us": round(kus["kpconv_fwd"], 2), "traffic": traffic("kpconv_fwd")}
    if rank == 0:
        # what this device delivers on plain streams, here and now: a fill and a copy of the size of the gather's output
        probe = torch.empty(stages[gi][2] // 4, dtype=torch.float32, device="cuda"); probe2 = torch.empty_like(probe)

        def _rate(fn, nbytes, reps=10):
            fn(); torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record(); torch.cuda.synchronize()
            return nbytes / (a.elapsed_time(b) / reps * 1e-3) / 1e9
        fill = _rate(lambda: probe.fill_(1.0), probe.numel() * 4)
        copy = _rate(lambda: probe2.copy_(probe), 2 * probe.numel() * 4)
        roofline.update({"measured_fill_GBps": round(fill, 1), "measured_copy_GBps": round(copy, 1), "frac_of_measured_fill": kgbps("queryandgroup") / fill})
        del probe, probe2
        if not args.no_gather_200k:
            try:
                roofline["gather_200k"] = gather_200k()
            except Exception as e:                                   # noqa: BLE001 — an extra measurement must not take the headline down
                roofline["gather_200k"] = {"error": repr(e)[:300]}
    out["roofline"] = roofline

    # ---- the forward block alone (round 1's step), timed the same way
    if backward:
        fstep = make_step(scene, k, False, args, overlap=not args.no_overlap, pipeline=pipeline)
        e_f = timed_region(fstep, args.steps, args.warmup, sync, D)
        out["forward_only"] = {"value": n * args.steps * world / e_f, "ms_per_step": e_f / args.steps * 1e3, "stages": " -> ".join(fstep.names), "issue": fstep.note}

    # ---- every step on its own (one hipGraph per step, no overlap between consecutive steps): the per-scene latency of the block
    if step.pipe is not None:
        nstep = make_step(scene, k, backward, args, overlap=True, pipeline=False)
        e_n = timed_region(nstep, args.steps, args.warmup, sync, D)
        out["no_pipeline"] = {"value": n * args.steps * world / e_n, "ms_per_step": e_n / args.steps * 1e3, "issue": nstep.note,
                              "note": "the headline value is pipelined THROUGHPUT (the search of step i+1 beside the rest of step i); this is one step at a time"}

    # ---- the same K steps with DDP's gradient all-reduce beside them (multi-rank runs)
    if (world > 1 or args.allreduce_single) and not args.no_allreduce:
        ar = GradAllReduce(args.allreduce_floats, "cuda")

        def step_ar():                                               # all-reduce of step i's gradients behind step i, beside step i+1 (as DDP's buckets)
            step(); step.join(); ar.finish(); ar.start()
        e_ar = timed_region(step_ar, args.steps, args.warmup, sync, D)

        def only_ar():
            ar.start(); ar.finish()
        e_only = timed_region(only_ar, args.steps, args.warmup, sync, D)
        nbytes = 4 * args.allreduce_floats
        out["grad_allreduce"] = {"value": n * args.steps * world / e_ar, "ms_per_step": e_ar / args.steps * 1e3, "bytes": nbytes,
                                 "allreduce_alone_ms": e_only / args.steps * 1e3,
                                 "allreduce_busbw_GBps": nbytes * 2 * (world - 1) / world / (e_only / args.steps) / 1e9, "ranks": world,
                                 "note": "one flat fp32 all-reduce of the reference network's 7,800,497 gradients per step over RCCL, started behind step i and "
                                         "joined behind step i+1, i.e. running beside the next step (what DDP adds, train.py:181-185); `value` above is the "
                                         "replica-only number"}
    if rank == 0 and world == 1 and not args.no_legs and (n, c, k) == (40960, 64, 16) and backward:
        del step
        torch.cuda.empty_cache()
        out.update(workload_legs(args))
    if rank == 0:
        if world == 1 and not args.no_cpu_baseline:
            from tests import cpu_baseline
            cb = cpu_baseline.run(n, c, k, seed=0, backward=backward)
            # north_star: KNN + group on the GPU against the host CPU's (search stage + gather, in-order stage times)
            gpu_kg = (stage_ms[names.index("knnquery_k%d" % k)] + kus["queryandgroup"] * 1e-3) * 1e-3
            kg = cb["knn_plus_group_seconds"]
            cb["knn_plus_group_speedup"] = {"gpu_seconds": gpu_kg, "vs_fastest_cpu_knn": (kg["knn_k%d_fastest_cpu" % k] + kg["queryandgroup_port"]) / gpu_kg,
                                            "vs_port_allcores": (kg["knn_k%d_port_allcores" % k] + kg["queryandgroup_port"]) / gpu_kg,
                                            "note": "GPU side = the step's whole search stage (it also carries the K=36 search) + the gather"}
            out["cpu_baseline"] = cb
        print(json.dumps(out), flush=True)
    return finish(world)



# ------------------------------------------------------------------------------------------------ C4 / C5 legs of the default line
def workload_legs(args):
    """The 1-GPU `--full` run of the default command line also measures BASELINE's other two single-GPU configurations —
    C4 (`--block pt`: the Point Transformer's vector-attention block) and C5 / C3-per-scene (`--workload convnet`) — each in a process of its own
    (own graphs, caches, scene) with the same timing contract, and appends a compact object per leg: {metric, value, ms_per_step, steps, roofline ...}.
    A leg that fails is reported as {"error": ...} and does not take the headline down."""
    import subprocess

    def leg(extra, pick):
        cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--full", "--no-cpu-baseline", "--no-legs"] + extra
        env = dict(os.environ)
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=420, env=env)
            lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not lines:
                return {"error": "rc %d: %s" % (r.returncode, (r.stderr or "").strip()[-300:]), "command": " ".join(cmd[1:])}
            d = json.loads(lines[-1])
            o = {k: d[k] for k in ("metric", "value", "unit", "ms_per_step", "steps", "warmup", "host_issue_ms_per_step", "dtype", "timed_regions_ms_per_step") if k in d}
            o["workload"] = d.get("config", {}).get("workload")
            o["issue"] = d.get("config", {}).get("issue")
            o["command"] = "python bench.py --full " + " ".join(extra)
            o.update(pick(d))
            return o
        except Exception as e:                                       # noqa: BLE001 — a leg must not take the headline down
            return {"error": repr(e)[:300], "command": " ".join(cmd[1:])}

    def pick_pt(d):
        r = d.get("roofline", {})
        return {"roofline": {k: r.get(k) for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "bytes_per_launch", "launch_us", "flops_per_launch",
                                                  "achieved_TFLOPs", "frac_of_f32_mfma_peak", "layer_bwd_us", "layer_bwd_note", "stage_ms") if k in r},
                "forward_only_ms_per_step": d.get("forward_only", {}).get("ms_per_step"),
                "no_pipeline_ms_per_step": (d.get("no_pipeline") or {}).get("ms_per_step"),
                "pipelined_ms_per_step": (d.get("pipelined") or {}).get("ms_per_step")}

    def pick_convnet(d):
        r = d.get("roofline", {})
        keep = {k: r.get(k) for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "bytes_per_launch", "launch_us", "stage_ms", "stage_sum_ms") if k in r}
        for sub in ("adaptive_weight", "adaptive_weight_bwd"):
            if sub in r:
                keep[sub] = {k: r[sub].get(k) for k in ("frac", "achieved", "launch_us", "bytes_per_launch", "frac_of_f32_vector_peak") if k in r[sub]}
        return {"roofline": keep, "no_pipeline_ms_per_step": (d.get("no_pipeline") or {}).get("ms_per_step"),
                "pipelined_ms_per_step": (d.get("pipelined") or {}).get("ms_per_step"),
                "ops_issued_from_python": {k: (d.get("pipelined_ops_issued_from_python") or {}).get(k) for k in ("ms_per_step", "host_issue_ms_per_step")},
                "native_call": {k: (d.get("pipelined_native_call") or {}).get(k) for k in ("ms_per_step", "host_issue_ms_per_step")},
                "timed_regions_ms_per_step": (d.get("pipelined") or {}).get("timed_regions_ms_per_step")}

    def tool_leg(script, extra, pick, timeout=240):
        """a measurement script of tools/ in a process of its own: its last JSON line, reduced by `pick`"""
        cmd = [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", script)] + extra
        env = dict(os.environ)
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
        try:
            t0 = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
            lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not lines:
                return {"error": "rc %d: %s" % (r.returncode, (r.stderr or "").strip()[-300:]), "command": "python tools/%s %s" % (script, " ".join(extra))}
            o = pick(json.loads(lines[-1]))
            o["command"] = "python tools/%s %s" % (script, " ".join(extra)); o["wall_s"] = round(time.perf_counter() - t0, 1)
            return o
        except Exception as e:                                       # noqa: BLE001
            return {"error": repr(e)[:300], "command": "python tools/%s %s" % (script, " ".join(extra))}

    def pick_train(d):
        seg = d.get("segments_ms") or {}
        ga = d.get("grad_allreduce") or {}
        return {"workload": d.get("workload"), "ms_per_step": d.get("ms_per_step"), "points_per_s": d.get("points_per_s"), "hipgraph": d.get("hipgraph"),
                "replay_ms": seg.get("replay_ms"), "allreduce_ms": seg.get("allreduce_ms"), "optimizer_ms": seg.get("optimizer_ms"),
                "launches_per_step": seg.get("launches_per_step", seg.get("graph_nodes")), "rccl_ranks": (d.get("ranks") or {}).get("rccl_ranks"),
                "backend": (d.get("ranks") or {}).get("backend"), "collective_issued": ga.get("collective_issued"), "gradient_bytes": ga.get("gradient_bytes"), "loss": d.get("loss")}

    def train_step():
        """config C4's full training step (PointTransformerSeg + CBL, 7.8 M parameters, forward + CE + CBL + backward + SGD) of one 40960-point scene as a replayed hipGraph,
        plain and through a one-rank RCCL group with the flat gradient reducer (the collective IS issued; not a scaling number)"""
        plain = tool_leg("bench_model.py", ["--graph", "--steps", "10", "--warmup", "3"], pick_train)
        group = tool_leg("bench_model.py", ["--graph", "--single-rank-group", "--steps", "10", "--warmup", "3"], pick_train)
        # the reference's own per-GPU batch (config/s3dis: batch_size 16 over 4 GPUs, tool/train.py:178): at one scene per step the sampler of the NEXT batch
        # (one workgroup per cloud, ~9 ms) is as long as the step it runs beside; four clouds sample side by side
        four = tool_leg("bench_model.py", ["--graph", "--scenes", "4", "--steps", "6", "--warmup", "2"], pick_train)
        o = {"plain": plain, "single_rank_group": group, "four_scenes": four}
        if plain.get("ms_per_step") and group.get("ms_per_step"):
            o["single_rank_group_over_plain"] = round(group["ms_per_step"] / plain["ms_per_step"], 3)
        return o

    def stage_shapes_leg():
        cmd = [sys.executable, os.path.abspath(__file__), "--workload", "stage_shapes"]
        env = dict(os.environ)
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
            lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not lines:
                return {"error": "rc %d: %s" % (r.returncode, (r.stderr or "").strip()[-300:]), "command": "python bench.py --workload stage_shapes"}
            d = json.loads(lines[-1]); d["command"] = "python bench.py --workload stage_shapes"
            return d
        except Exception as e:                                       # noqa: BLE001
            return {"error": repr(e)[:300], "command": "python bench.py --workload stage_shapes"}

    steps = str(min(args.steps, 30)); warm = str(min(args.warmup, 5))
    return {"train_step": train_step(), "stage_shapes": stage_shapes_leg(),
            "pt_block": leg(["--block", "pt", "--steps", steps, "--warmup", warm], pick_pt),
            # the ConvNet step is issued eagerly by two host threads: short timed regions (20 steps = 60 ms) caught the threads' start-up in two of four runs
            # (3.1 or 3.6-4.1 ms per step); 40 steps and 5 warm-up steps cost 0.3 s more
            "convnet": leg(["--workload", "convnet", "--steps", "40", "--warmup", "5"], pick_convnet)}

# ------------------------------------------------------------------------------------------------ ConvNet workload (BASELINE configs C5 / C3)
def run_convnet(args, D, world, rank, local):
    """python bench.py --workload convnet: one step = the radius / grid pyramid of one resident N-point cloud (13 radius searches + 4 grid
    subsamplings), AdaptiveWeight forward + backward on its 5 layers at C = 72 ... 1152, scene labels and the TF-side CBL forward + backward
    on every layer (contrastboundary_amd/convnet_path.py).  Issued eagerly: the layer sizes are data dependent (one host sync per grid
    subsampling, as the TF op's dynamic output shape)."""
    torch.cuda.set_device(local)
    D.init("nccl" if world > 1 else None)
    if world > 1:
        import torch.distributed as dist
        assert dist.get_world_size() == args.gpus, "RCCL process group has %d ranks, --gpus says %d" % (dist.get_world_size(), args.gpus)
    from contrastboundary_amd import convnet_path as CP, local_aggregation as LA, tf_ops
    n = args.points
    backward = not args.forward_only
    scene = CP.ConvNetScene(n, seed=rank, b=1)
    stage_list = CP.stages(scene, backward=backward)
    names = [s[0] for s in stage_list]
    state = {}

    def step():
        CP.run_once(scene, state, stage_list=stage_list)
    t = time.perf_counter()
    while time.perf_counter() - t < 0.5:                              # settle: code objects, workspaces, clocks
        step(); torch.cuda.synchronize()
    elapsed = timed_region(step, args.steps, args.warmup, torch.cuda.synchronize, D)
    in_order = {"ms_per_step": elapsed / args.steps * 1e3, "value": n * args.steps * world / elapsed,
                "host_issue_ms_per_step": timed_region.issue_s / args.steps * 1e3, "issue": "eager, every stage in order on one stream and one host thread"}
    pipelined = pipelined_ops = native = None
    if not args.no_pipeline:
        # the pyramid is input-pipeline work (tf.data workers + prefetch in the reference): a loader thread builds the NEXT step's pyramid through the
        # native per-layer calls (no interpreter lock held) on a stream of its own, beside the layers of this step.  Every step still builds one pyramid
        # and runs one model pass; the timed region closes after the loader has issued, and the device has finished, everything (K + 1 pyramids started
        # inside or before it, K of them consumed: the first was built before t0, the last is waited for).
        loader = CP.PyramidLoader(scene)
        p_stages = CP.stages(scene, backward=backward, loader=loader)
        p_state = {}

        def p_step():
            CP.run_once(scene, p_state, stage_list=p_stages)

        def p_sync():
            loader.drain(); torch.cuda.synchronize()
        for _ in range(3):
            p_step()
        p_sync()
        loader.waited_s = 0.0
        e_p, p_regions = timed_median(p_step, args.steps, args.warmup, p_sync, D)
        waited = loader.waited_s / (3 * args.steps + args.warmup) * 1e3      # the loader's take() blocks while the pyramid is still being issued: waiting, not issuing
        pipelined = {"ms_per_step": e_p / args.steps * 1e3, "value": n * args.steps * world / e_p, "timed_regions_ms_per_step": p_regions,
                     "host_issue_ms_per_step": max(timed_region.issue_s / args.steps * 1e3 - waited, 0.0), "host_wait_for_loader_ms_per_step": waited,
                     "issue": "eager: loader threads (convnet_path.PyramidLoader, %d pyramids in flight, a thread and stream each: the input pipeline's prefetch) build the "
                              "coming steps' pyramids (one native cbl_pyramid call each) beside this step's layers, issued op by op from Python" % loader.depth}
        loader.close()
        if e_p < elapsed:
            elapsed = e_p
        # the same step with every layer's work issued by ONE native call (cbl_convnet_step: the same kernels in the same order, no interpreter / autograd
        # engine / allocator between the ~70 launches) beside the loader thread's pyramid: the main thread's issue time is two calls per step
        loader = CP.PyramidLoader(scene)
        n_stages = CP.native_stages(scene, loader=loader)
        n_state = {}

        def n_step():
            CP.run_once(scene, n_state, stage_list=n_stages)

        def n_sync():
            loader.drain(); torch.cuda.synchronize()
        for _ in range(3):
            n_step()
        n_sync()
        loader.waited_s = 0.0
        e_n, n_regions = timed_median(n_step, args.steps, args.warmup, n_sync, D)
        waited = loader.waited_s / (3 * args.steps + args.warmup) * 1e3
        native = {"ms_per_step": e_n / args.steps * 1e3, "value": n * args.steps * world / e_n, "timed_regions_ms_per_step": n_regions,
                  "host_issue_ms_per_step": max(timed_region.issue_s / args.steps * 1e3 - waited, 0.0), "host_wait_for_loader_ms_per_step": waited,
                  "issue": "two native calls per step: loader threads (%d pyramids in flight, a thread and stream each) build the coming steps' pyramids (cbl_pyramid) "
                           "beside ONE cbl_convnet_step call that issues every layer's AdaptiveWeight forward + backward, scene labels and contrast head "
                           "(convnet_path.NativeLayers; tests/test_gpu_bench_convnet.py: bit-identical to the op-by-op step)" % loader.depth}
        loader.close()
        pipelined_ops = pipelined
        # the reported step IS the native-call one (the design of this path; its issue time is what `host_issue_ms_per_step` is asked about) unless it
        # measures clearly slower than the op-by-op issue of the same kernels (then that one, and both are in the line either way)
        if e_n <= 1.05 * elapsed:
            elapsed, pipelined = e_n, native
    spread = rank_spread(D)
    pyr = state["pyr"]
    sizes = [int(p.shape[0]) for p in pyr["points"]]
    widths = [int(nb.shape[1]) for nb in pyr["neighbors"]]
    out = {"ranks": spread, "metric": "points/sec through radius+grid pyramid, AdaptiveWeight fwd+bwd (5 layers) and TF-side CBL, ConvNet N=%d" % n,
           "value": n * args.steps * world / elapsed, "unit": "points/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": elapsed / args.steps * 1e3,
           "host_issue_ms_per_step": (pipelined if pipelined is not None and pipelined["ms_per_step"] <= in_order["ms_per_step"] else in_order)["host_issue_ms_per_step"],
           "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic", "no_pipeline": in_order, "pipelined": pipelined,
           "pipelined_ops_issued_from_python": pipelined_ops, "pipelined_native_call": native,
           "config": {"workload": "ConvNet per-scene work (BASELINE configs C5 / C3): S-room scaled to %d points, dl0=%.2f, density %.0f, %d layers, "
                                  "limits %s; layer sizes %s, neighbour widths %s, AdaptiveWeight widths %s, CBL on a %d-d latent; stages: %s"
                                  % (n, CP.DL0, CP.DENSITY, scene.layers, CP.LIMITS[:scene.layers], sizes, widths, scene.widths, CP.CBL_DIM, " -> ".join(names)),
                      "parallelism": "scene-per-GPU replicas x%d (no data-path collective)" % world,
                      "issue": ((pipelined["issue"] if pipelined is not None and pipelined["ms_per_step"] <= in_order["ms_per_step"] else in_order["issue"])
                                + "; data-dependent layer sizes: one host wait per grid subsampling, like the TF op's dynamic shape")}}
    if args.no_extra or not args.full:
        if rank == 0:
            print(json.dumps(out), flush=True)
        return finish(world)

    # ---- per-stage device times: HIP events on the launch stream around every stage of in-order steps
    samples = []
    for _ in range(7):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in stage_list]
        for (a, b), (_, fn, _, _) in zip(ev, stage_list):
            a.record(); fn(state); b.record()
        torch.cuda.synchronize()
        samples.append([a.elapsed_time(b) for a, b in ev])
    stage_ms = [float(v) for v in np.median(np.asarray(samples[2:]), axis=0)]
    stage_bytes = [int(s[2](state)) for s in stage_list]

    # ---- the two roofline kernels, each alone: back-to-back launches behind a filler, two events around the run
    filler = torch.empty(1 << 32, dtype=torch.uint8, device="cuda")

    def alone(fn, reps=10):
        fn(); fn(); torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        filler.fill_(0); filler.fill_(1)
        a.record()
        for _ in range(reps):
            fn()
        b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e3                         # us
    pts0, len0, nb0 = pyr["points"][0], pyr["batches_len"][0], pyr["neighbors"][0]
    r0 = CP.DL0 * CP.DENSITY / 2.0
    arr0 = scene.layer_arrays(0, sizes[0])
    c0, k0 = scene.widths[0], widths[0]
    us_radius = alone(lambda: tf_ops.tf_batch_neighbors(pts0, pts0, len0, len0, r0, CP.LIMITS[0], exact_shape=False))
    us_aw = alone(lambda: LA.adaptive_weight(pts0, pts0, nb0, arr0["feat"], r0, scene.fc_weight[0], scene.fc_bias[0], "mean"))
    f_l = arr0["feat"].detach().requires_grad_(True); w_l = scene.fc_weight[0].detach().requires_grad_(True); b_l = scene.fc_bias[0].detach().requires_grad_(True)
    o_l = LA.adaptive_weight(pts0, pts0, nb0, f_l, r0, w_l, b_l, "mean")
    us_aw_bwd = alone(lambda: torch.autograd.grad(o_l, (f_l, w_l, b_l), arr0["grad"], retain_graph=True)) if backward else None
    del filler
    rb = CP.radius_bytes(sizes[0], sizes[0], CP.LIMITS[0])
    ab = CP.adaptive_weight_bytes(sizes[0], sizes[0], k0, c0)
    gb = lambda nbytes, us: nbytes / (us * 1e-6) / 1e9
    roofline = {"kernel": "radius_group_kernel (layer 0: %d queries x %d supports, r=%.2f, limit %d) incl. its grid build" % (sizes[0], sizes[0], r0, CP.LIMITS[0]),
                "stage": "radius search of layer 0", "bound": "hbm", "achieved": gb(rb, us_radius), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": gb(rb, us_radius) / HBM_PEAK_GBS, "traffic": None, "bytes_per_launch": rb, "launch_us": round(us_radius, 2),
                "note": "achieved = SURVEY 8(d) N2 bytes (12 Nq + 12 Ns + 4 Nq limit) / HIP-event duration of 10 back-to-back calls of the search alone / 10",
                "adaptive_weight": {"kernel": "adaptive_weight forward, layer 0 (n=%d, K=%d, C=%d)" % (sizes[0], k0, c0), "bound": "hbm", "achieved": gb(ab, us_aw),
                                    "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gb(ab, us_aw) / HBM_PEAK_GBS, "bytes_per_launch": ab, "launch_us": round(us_aw, 2),
                                    "gathered_bytes_per_launch": 4 * sizes[0] * k0 * c0,
                                    "gathered_GBps": gb(4 * sizes[0] * k0 * c0, us_aw),
                                    "flops_per_launch": CP.adaptive_weight_flops(sizes[0], k0, c0),
                                    "achieved_TFLOPs": CP.adaptive_weight_flops(sizes[0], k0, c0) / (us_aw * 1e-6) / 1e12,
                                    "frac_of_f32_vector_peak": CP.adaptive_weight_flops(sizes[0], k0, c0) / (us_aw * 1e-6) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                                    "measured_bound": "VALU issue slots, not memory (profiles/r03_aw_lane_width_sweep.md: more rows in flight per lane made it slower; "
                                                      "instruction count x 4 clk / SIMD accounts for the time)",
                                    "note": "SURVEY 8(d) a14 bytes 12n + 12n0 + 4 n0 C + 4 n K + 4 n C; gathered = the n K C floats the kernel pulls through L2"},
                "stage_ms": {names[i]: round(stage_ms[i], 4) for i in range(len(names))},
                "stage_sum_ms": round(float(sum(stage_ms)), 4),
                "stage_algorithmic_GBps": {names[i]: round(stage_bytes[i] / (stage_ms[i] * 1e-3) / 1e9, 1) for i in range(len(names)) if stage_ms[i] > 0}}
    if us_aw_bwd is not None:
        bb = ab + 4 * sizes[0] * c0
        roofline["adaptive_weight_bwd"] = {"bound": "hbm", "achieved": gb(bb, us_aw_bwd), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gb(bb, us_aw_bwd) / HBM_PEAK_GBS,
                                           "bytes_per_launch": bb, "launch_us": round(us_aw_bwd, 2)}
    out["roofline"] = roofline
    if rank == 0:
        if world == 1 and not args.no_cpu_baseline:
            from tests import cpu_baseline
            out["cpu_baseline"] = cpu_baseline.run_convnet(n, seed=0, gpu_pyramid_ms=stage_ms[0])
        print(json.dumps(out), flush=True)
    return finish(world)


# ------------------------------------------------------------------------------------------------ Point Transformer block (a1 + a3 + a4 + a8)
def layer_backward_graph_us(layer, scene, idx, reps=20):
    """the attention layer's backward as a replayed hipGraph, on a COPY of the layer (fresh parameters: their gradient accumulators are created on the
    capture stream — a capture that meets accumulators of another stream crashes on ROCm 7.2, see Step.capture)"""
    import copy
    import gc
    try:
        lay = copy.deepcopy(layer).train()
        params = list(lay.parameters())
        g_up = scene.upstream(idx.shape[1])["grad_kpconv"]
        gc.collect()
        st = {}

        def fwd():
            st["x"] = scene.feat.detach().requires_grad_(True)
            st["y"] = lay([scene.xyz, st["x"], scene.offset], idx=idx)

        def bwd():
            st["g"] = torch.autograd.grad(st["y"], [st["x"]] + params, g_up, retain_graph=True)
        cap = torch.cuda.Stream(); cap.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(cap):
            for _ in range(3):
                fwd(); bwd()
        torch.cuda.current_stream().wait_stream(cap); torch.cuda.synchronize()
        gf, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(gf, capture_error_mode="thread_local"):
            fwd()
        with torch.cuda.graph(gb, capture_error_mode="thread_local"):
            bwd()
        gf.replay(); gb.replay(); torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            gb.replay()
        b.record(); torch.cuda.synchronize()
        us = a.elapsed_time(b) / reps * 1e3
        del gf, gb, st
        return round(us, 2)
    except Exception as e:                                           # noqa: BLE001 - a measurement beside the leg must not take it down
        torch.cuda.synchronize()
        return {"error": "%s: %s" % (type(e).__name__, str(e)[:120])}


def graph_us(fn, reps=20, warm=3):
    """device time of fn() as a replayed hipGraph: `reps` replays between two HIP events / reps (a graph's launch gaps, no host issue time)"""
    cap = torch.cuda.Stream(); cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cap):
        for _ in range(warm):
            fn()
    torch.cuda.current_stream().wait_stream(cap); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        fn()
    g.replay(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def run_stage_shapes(args, local):
    """python bench.py --workload stage_shapes: the north-star gather (a3), the attention layer (a4, forward and backward) and the sampler (a2) at the five REAL
    stage shapes of the reference's Point Transformer — (n, K, C) = (40960, 8, 32) (10240, 16, 64) (2560, 16, 128) (640, 16, 256) (160, 16, 512),
    /root/reference/pytorch/model/pointtransformer_seg.py:35,49-58 — on an S-room scene whose stages are this build's own FPS (stride 4).  Gather and layer
    times are replayed hipGraphs (device time, no host issue time); FPS is one eager call between two events (milliseconds of one workgroup)."""
    import gc
    torch.cuda.set_device(local)
    torch.backends.cuda.preferred_blas_library("cublas")
    from contrastboundary_amd import blocks, pointops, synthetic as S
    dev = "cuda"
    shapes = [(40960, 8, 32), (10240, 16, 64), (2560, 16, 128), (640, 16, 256), (160, 16, 512)]
    xyz = torch.from_numpy(S.s_room(40960, 0)[0]).to(dev)
    p, o, fps_us = [xyz], [torch.tensor([40960], dtype=torch.int32, device=dev)], [None]
    for i in range(1, 5):
        no = torch.tensor([shapes[i][0]], dtype=torch.int32, device=dev)
        ts = []
        for r in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); a.record()
            idx = pointops.furthestsampling(p[i - 1], o[i - 1], no)
            b.record(); torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        fps_us.append(float(np.median(ts[1:])))
        p.append(p[i - 1][idx.long()].contiguous()); o.append(no)
    rows = []
    for i, (n, K, C) in enumerate(shapes):
        torch.manual_seed(100 + i)
        feat = torch.randn(n, C, device=dev)
        g_up = torch.randn(n, C, device=dev)
        idx, _ = pointops.knnquery(K, p[i], p[i], o[i], o[i])
        row = {"stage": i, "n": n, "K": K, "C": C}
        gb = 4 * n * K + 12 * n + 12 * n + 4 * n * C + 4 * n * K * (3 + C)
        try:
            us = graph_us(lambda: pointops.queryandgroup(K, p[i], p[i], feat, idx, o[i], o[i], use_xyz=True))
            row["queryandgroup_us"] = round(us, 2); row["queryandgroup_GBps"] = round(gb / (us * 1e-6) / 1e9, 1); row["queryandgroup_frac_of_8TBps"] = round(gb / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 3)
            layer = blocks.PointTransformerLayer(C, C, 8, K).to(dev).train()
            params = list(layer.parameters())
            gc.collect()
            st = {}

            def fwd():
                st["x"] = feat.detach().requires_grad_(True)
                st["y"] = layer([p[i], st["x"], o[i]], idx=idx)

            def bwd():
                st["g"] = torch.autograd.grad(st["y"], [st["x"]] + params, g_up, retain_graph=True)
            cap = torch.cuda.Stream(); cap.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(cap):                              # the layer's first use, the transposed table, the gradient accumulators: all on the capture stream
                for _ in range(2):
                    fwd(); bwd()
            torch.cuda.current_stream().wait_stream(cap); torch.cuda.synchronize()
            row["pt_layer_fwd_us"] = round(graph_us(fwd, warm=1), 2)
            row["pt_layer_bwd_us"] = round(graph_us(bwd, warm=1), 2)
            del st, layer, params
        except Exception as e:                                       # noqa: BLE001 - report what was measured
            row["error"] = "%s: %s" % (type(e).__name__, str(e)[:120])
            torch.cuda.synchronize()
        if fps_us[i] is not None:
            row["fps_from_prev_us"] = round(fps_us[i], 1)
        rows.append(row)
    out = {"workload": "stage_shapes", "scene": "S-room(40960, seed 0), stages by this build's FPS (stride 4)", "device": torch.cuda.get_device_name(0),
           "timing": "queryandgroup / pt_layer: 20 replays of a hipGraph of the call between two HIP events / 20; fps: one eager call between two events, median of 2",
           "pt_layer": "blocks.PointTransformerLayer(C, C, share_planes 8, nsample K), train mode: q / k / v projections + the fused attention passes; backward w.r.t. the input features and all parameters (transposed table already built)",
           "stages": rows}
    print(json.dumps(out), flush=True)
    return 0


def run_pt(args, D, world, rank, local):
    """python bench.py --block pt: the block with the Point Transformer's vector-attention layer (pytorch/model/blocks.py:31-44) as its local
    aggregation — KNN -> PointTransformerLayer (q/k/v, linear_p, attention over the K neighbours, softmax, aggregation; forward + backward
    w.r.t. features and all parameters) -> CBL head.  Same issue modes, timing and checks as the KPConv block; `roofline` is the layer's forward
    (its attn_* kernels + the dense q/k/v) against SURVEY 8(d)'s a4 bytes / flops, timed alone as a replayed hipGraph."""
    torch.cuda.set_device(local)
    D.init("nccl" if world > 1 else None)
    if world > 1:
        import torch.distributed as dist
        assert dist.get_world_size() == args.gpus
    torch.backends.cuda.preferred_blas_library("cublas")             # rocBLAS for the q/k/v Linear layers (tools/bench_model.py: 2-20x hipBLASLt here)
    from contrastboundary_amd import hotpath
    n, c, k = args.points, args.channels, args.k
    backward = not args.forward_only
    scene = hotpath.Scene.synthetic(n, c, seed=rank, b=1)
    pipeline = not (args.no_pipeline or args.no_overlap or args.no_nested or args.no_graph)
    step, pipe_check = checked_pipeline_step(scene, k, backward, args, overlap=not args.no_overlap, pipeline=pipeline)
    sync = torch.cuda.synchronize
    elapsed, regions = timed_headline(step, args, sync, D)
    out = {"ranks": rank_spread(D), "pipeline_check": pipe_check, "timed_regions_ms_per_step": regions, "timed_regions_note": REGIONS_NOTE[args.full],
           "metric": "points/sec through KNN+group+PointTransformer(vector attention)+CBL block, S3DIS N=%d K=%d" % (n, k),
           "value": n * args.steps * world / elapsed, "unit": "points/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": elapsed / args.steps * 1e3, "host_issue_ms_per_step": timed_region.issue_s / args.steps * 1e3, "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": "S3DIS-shaped synthetic scene (S-room), N=%d, K=%d, C=%d, 1 scene per GPU per step, %s; stages: %s"
                                  % (n, k, c, "forward + backward of the block" if backward else "forward block + CBL head", " -> ".join(step.names)),
                      "block": "Point Transformer layer (blocks.py:31-44: share_planes 8, train-mode BatchNorms, seeded weights) in place of KPConv",
                      "parallelism": "scene-per-GPU replicas x%d (no data-path collective)" % world, "issue": step.note}}
    if args.dump_outputs and rank == 0:
        out["dumped_outputs"] = dump_outputs(step.last_state(), n, args.dump_outputs)
    if args.no_extra or not args.full:
        if rank == 0:
            print(json.dumps(out), flush=True)
        return finish(world)
    st_in, stage_ms, how = stage_times(scene, k, backward, args)
    names, stages = st_in.names, st_in.stages
    # the layer's forward alone: one hipGraph of it, replayed back to back between two HIP events
    layer = hotpath.pt_layer(scene)
    from contrastboundary_amd import pointops
    # inside ONE neighbour cache: the cell order the search registers (the layer's processing order) lives as long as the cache that owns it — measured outside,
    # the layer walks its tiles in index order: 142 / 313 us instead of 132 / 272 us forward / backward
    with pointops.neighbor_cache():
        idx, _ = pointops.knnquery_raw(k, scene.xyz, scene.xyz, scene.offset, scene.offset)
        with torch.no_grad():
            us = graph_us(lambda: layer([scene.xyz, scene.feat, scene.offset], idx=idx))
        bwd_us = layer_backward_graph_us(layer, scene, idx) if backward else None
    li = names.index("pt_layer_fwd")
    nbytes, flops = stages[li][2], stages[li][3]
    out["roofline"] = {"kernel": "PointTransformerLayer forward (csrc/pt_layer.hip + cbl_triple_linear): q/k/v projections (1 launch), p chain, BN_c statistics, w2 on MFMA tiles, softmax, aggregation; 3 BatchNorm finalizes",
                       "stage": "pt_layer_fwd", "bound": "hbm", "achieved": nbytes / (us * 1e-6) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                       "frac": nbytes / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, "traffic": None, "bytes_per_launch": nbytes, "launch_us": round(us, 2),
                       "flops_per_launch": flops, "achieved_TFLOPs": flops / (us * 1e-6) / 1e12, "frac_of_f32_mfma_peak": flops / (us * 1e-6) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                       "note": "SURVEY 8(d) a4 (idx given): bytes 12n + 12nC + 4nK + 4nC, flops 2nK(9 + 3C + C^2/8 + C^2/64) + 6nC^2; duration = 20 replays of a "
                               "hipGraph of the layer's forward alone between two HIP events / 20.  stage_ms: " + how,
                       "stage_ms": {names[i]: round(stage_ms[i], 4) for i in range(len(stages))}, "stage_sum_ms": round(float(sum(stage_ms)), 4)}
    if bwd_us is not None:
        out["roofline"]["layer_bwd_us"] = bwd_us                     # float, or {"error": ...}
        out["roofline"]["layer_bwd_note"] = ("the layer's backward alone (w.r.t. its input features and all parameters, the transposed table already built): 20 replays of a hipGraph "
                                             "between two HIP events / 20 — device time with a graph's launch gaps and one replay's fixed cost (stage_ms.pt_layer_bwd: the same chain inside the in-order step, by difference of prefix graphs)")
    if backward:
        fstep = make_step(scene, k, False, args, overlap=not args.no_overlap, pipeline=pipeline)
        e_f = timed_region(fstep, args.steps, args.warmup, sync, D)
        out["forward_only"] = {"value": n * args.steps * world / e_f, "ms_per_step": e_f / args.steps * 1e3, "stages": " -> ".join(fstep.names)}
    if step.pipe is not None:
        nstep = make_step(scene, k, backward, args, overlap=True, pipeline=False)
        e_n = timed_region(nstep, args.steps, args.warmup, sync, D)
        out["no_pipeline"] = {"value": n * args.steps * world / e_n, "ms_per_step": e_n / args.steps * 1e3, "issue": nstep.note}
        if e_n < elapsed:
            # this block's backward is one long chain: two steps in flight contend more than they overlap (measured 1.45 vs 1.38 ms).  The line
            # reports the faster issue mode and keeps the other beside it.
            out["pipelined"] = {"value": out["value"], "ms_per_step": out["ms_per_step"], "issue": out["config"].get("issue")}
            out["value"], out["ms_per_step"] = out["no_pipeline"]["value"], out["no_pipeline"]["ms_per_step"]
            out["config"]["issue"] = nstep.note + " (one step at a time: faster than the software pipeline for this block)"
    if rank == 0:
        print(json.dumps(out), flush=True)
    return finish(world)


def finish(world):
    import torch.distributed as tdist
    if tdist.is_available() and tdist.is_initialized():
        tdist.destroy_process_group()
    return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse(argv)
    if args.dump_outputs and (args.workload != "block" or args.host_dry_run):
        sys.stderr.write("bench.py: --dump-outputs writes the outputs of the block's step (the default workload, --block pt)\n")
        return 2
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return spawn(args, argv)
    from contrastboundary_amd import distributed as D
    world, rank, local = D.env_world()
    if world != args.gpus:
        sys.stderr.write("bench.py: WORLD_SIZE=%d but --gpus %d\n" % (world, args.gpus))
        return 2
    if args.host_dry_run:
        return host_dry_run(args, D, world, rank)
    if not torch.cuda.is_available():
        sys.stderr.write("bench.py: no GPU visible (the hot path has no CPU fallback)\n")
        return 2
    if args.workload == "stage_shapes":
        return run_stage_shapes(args, local)
    return (run_convnet if args.workload == "convnet" else run_pt if args.block == "pt" else run_gpu)(args, D, world, rank, local)


if __name__ == "__main__":
    sys.exit(main())
