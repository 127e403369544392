"""The ten entries of contrastboundary_amd/csrc/attention.hip ON THE DEVICE against the float64 oracle of tests/attention_oracle.py — the mathematics, not
another kernel: cbl_attn_w2_forward (training and evaluation), cbl_attn_agg_forward / _softmax_forward, and the two backward passes through their scatter entries
(float atomics) and through the gather entry of the width (_csr at C = 32 / 64, _wide_csr at 128 / 256 / 512), with and without an `order`.  Every scene is
flip-free (O.make_flip_free), every entry of every output is compared under the 1e-4 contract (O.close, which prints the worst ratio), nothing is excluded.
Called through ctypes as tests/test_gpu_deterministic.py does: outputs pre-filled with NaN (zeros where a scatter entry accumulates), a workspace of exactly
cbl_attn_workspace_bytes bytes.  tests/test_attention_oracle_host.py runs the same driver and oracle on the host-emulated library.

The scenes, (n, K, C).  EDGE: the tile and width edges.  CAPS: one point more trips than one — every pass that writes a partial row per workgroup
(attn_w2_stats, _bwd_reduce, _bwd_apply, attn_agg_backward and their wide twins; also attn_w2_forward_kernel and the wide gathers) is launched on at_blocks(n, C)
workgroups = min(points / points per workgroup, cap), cap = AT_MAX_BLOCKS = 1024 workgroups of 256 / C points at C = 32 / 64 (8192 / 4096 points), and
at_wide_blocks(C) = 2048 / 768 / 256 workgroups of one point at C = 128 / 256 / 512.  Past the cap the grid-stride loop takes a second trip and a workgroup's
partial row sums several points; each n passes its cap by a count that is no multiple of the points per trip.  The remaining caps are named at their lists."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import attention_oracle as O

pytestmark = pytest.mark.gpu

EDGE = [(41, 8, 32),          # a flat MFMA tile holds two points; n K is no multiple of 16
        (50, 1, 64),          # K = 1
        (33, 17, 64),         # two tiles per point, one pair in the second
        (19, 64, 64),         # K = 64, the largest attention.supported() admits
        (37, 5, 128),         # a ragged K at a wide width
        (23, 16, 256),        # wide, the stages' own K
        (17, 33, 512),        # K over 32 at the widest width
        (9, 64, 256)]         # K = 64 at a wide width
CAPS = [(8300, 8, 32),        # over 1024 x 8 = 8192 points
        (4200, 16, 64),       # over 1024 x 4 = 4096
        (2100, 16, 128),      # over 2048
        (800, 16, 256),       # over 768
        (2600, 8, 256),       # over 768 three times and a part: the points of a 4-scene batch
        (300, 16, 512)]       # over 256
ALL = EDGE + CAPS
# attn_w2_forward_mfma_kernel: min(tiles / 4, 8192) workgroups of 4 waves, a 16-pair tile per wave and trip -> a second trip beyond 32768 tiles.
# K = 17: two tiles per point, 33000 tiles; K = 16: one flat tile per point, 33000 tiles
MFMA_GRADS, MFMA_FORWARD = (16500, 17, 32), (33000, 16, 32)
# attn_agg_forward: no partial rows, a grid of its own — cbl_grid_for(n C, 256, 4096) workgroups of 256 / C points at C <= 64 (64: 16384 points), min(n, 2048) above
AGG_FORWARD_GRID = [(16500, 8, 64), (2100, 8, 512)]
# the narrow gathers over the transposed table: cbl_grid_for(n C, 256, 8192) workgroups of 256 / C targets (C = 64: 32768 targets)
NARROW_GATHER_GRID = (33000, 8, 64)
WITH_GRADIENTS = set(ALL + [MFMA_GRADS])
FORMS = ["scatter", "index order", "ordered"]


class DeviceBackend:
    """device tensors for O.Entries; `shift` floats into a buffer whose start torch aligns to 256 bytes and more"""

    @property
    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def put(self, array, shift=0):
        t = torch.from_numpy(np.ascontiguousarray(array))
        raw = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
        out = raw[shift:shift + t.numel()].view(t.shape)
        out.copy_(t)
        assert (out.data_ptr() % 16 == 0) == (shift == 0)
        return out

    def fill(self, shape, value, dtype=np.float32):
        return torch.full(tuple(shape), value, dtype={np.float32: torch.float32, np.uint8: torch.uint8, np.int64: torch.int64}[dtype], device="cuda")

    def ptr(self, buf):
        return None if buf is None else ctypes.c_void_p(buf.data_ptr())

    def get(self, buf):
        return buf.cpu().numpy()                                       # (synchronises)


@pytest.fixture(scope="module")
def entries():
    from contrastboundary_amd import _lib
    return O.Entries(_lib.lib(), DeviceBackend())


class Scene:
    """a shape's inputs and its float64 results, each computed once per module and left unchanged"""

    def __init__(self, n, K, C):
        self.tag = "(%d, %d, %d)" % (n, K, C)
        self.idx, self.a, self.touched, self.rounds = O.case(n, K, C, gradients=(n, K, C) in WITH_GRADIENTS)

    @functools.cached_property
    def w2(self):
        ref = O.reference_w2(self.idx, self.a)
        ref.pop("z")
        return ref

    @functools.cached_property
    def w2_eval(self):
        return O.reference_w2(self.idx, self.a, training=False)["w2"]

    @functools.cached_property
    def agg(self):
        return [O.reference_agg(self.idx, self.a, softmax) for softmax in (0, 1)]

    @functools.cached_property
    def tables(self):
        return dict(O.tables(self.idx, self.idx.size), scatter=None)


@functools.lru_cache(maxsize=None)
def scene_of(n, K, C):
    return Scene(n, K, C)


# ---------------------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("n,K,C", ALL + [MFMA_GRADS, MFMA_FORWARD])
def test_logits_forward_training(entries, n, K, C):
    """w2, the saved mean and invstd, both running statistics (from buffers that are not 0 / 1) and num_batches_tracked"""
    s = scene_of(n, K, C)
    O.check_w2_forward(entries.w2_forward(s.idx, s.a, True), s.w2, s.tag + " train")


@pytest.mark.parametrize("n,K,C", ALL + [MFMA_GRADS, MFMA_FORWARD])
def test_logits_forward_evaluation(entries, n, K, C):
    s = scene_of(n, K, C)
    O.close(entries.w2_forward(s.idx, s.a, False)["w2"], s.w2_eval, s.tag + " eval w2")


@pytest.mark.parametrize("n,K,C", [c for c in ALL if c[2] <= 64])
def test_logits_forward_with_unaligned_rows(entries, n, K, C):
    """x_q / x_k one float past a 16-byte boundary: cbl_attn_w2_forward then leaves the MFMA kernel's float4 loads for attn_w2_forward_kernel (DPP group sums;
    on at_blocks workgroups, so the two CAPS scenes also take its second trip).  No caller in the package does this; same oracle, same bound.  Only this entry:
    the other narrow kernels read scalars, the wide ones were not checked for alignment."""
    s = scene_of(n, K, C)
    O.check_w2_forward(entries.w2_forward(s.idx, s.a, True, unaligned=True), s.w2, s.tag + " train, unaligned rows")


@pytest.mark.parametrize("softmax", [0, 1])
@pytest.mark.parametrize("n,K,C", ALL + AGG_FORWARD_GRID)
def test_aggregation_forward(entries, n, K, C, softmax):
    s = scene_of(n, K, C)
    got = entries.agg_forward(s.idx, s.a, softmax)
    O.close(got["out"], s.agg[softmax]["out"], "%s agg softmax %d out" % (s.tag, softmax))
    if softmax:
        O.close(got["weights"], s.agg[1]["weights"], s.tag + " agg softmax weights")


# ---------------------------------------------------------------------------------------------------------------- 2. backward
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n,K,C", ALL + [MFMA_GRADS])
def test_logits_backward(entries, n, K, C, form):
    """the nine gradients from the oracle's mean / invstd (rounded to fp32, as the forward pass saves them); the gather entries write grad x_k over a NaN fill,
    exact zeros for the target nobody lists"""
    s = scene_of(n, K, C)
    got = entries.w2_backward(s.idx, s.a, s.w2["mean"], s.w2["invstd"], s.tables[form])
    O.check_w2_backward(got, s.w2, "%s w2 backward, %s" % (s.tag, form), form != "scatter")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("softmax", [0, 1])
@pytest.mark.parametrize("n,K,C", ALL + [NARROW_GATHER_GRID])
def test_aggregation_backward(entries, n, K, C, softmax, form):
    """the five gradients; with the softmax the entry is given the oracle's softmax weights (rounded to fp32) and returns the gradient of the logits"""
    s = scene_of(n, K, C)
    ref = s.agg[softmax]
    got = entries.agg_backward(s.idx, s.a, ref["weights"], softmax, s.tables[form])
    O.check_agg_backward(got, ref, "%s agg backward softmax %d, %s" % (s.tag, softmax, form), form != "scatter", softmax, s.a["g_out"])


# ---------------------------------------------------------------------------------------------------------------- 3. the autograd wrappers
BACKWARD_ENTRIES = {"cbl_attn_w2_backward", "cbl_attn_w2_backward_csr", "cbl_attn_w2_backward_wide_csr", "cbl_attn_agg_backward", "cbl_attn_agg_softmax_backward",
                    "cbl_attn_agg_backward_csr", "cbl_attn_agg_backward_wide_csr"}


@pytest.fixture
def counted(monkeypatch):
    from contrastboundary_amd import _lib
    from tests.test_gpu_deterministic import CountingLib
    proxy = CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: proxy)
    return proxy.calls


@pytest.mark.parametrize("switch", [False, True])
@pytest.mark.parametrize("n,K,C", [(4200, 16, 64), (300, 16, 512)])
def test_autograd_wrappers(counted, n, K, C, switch):
    """attention.AttnW2 / AttnAgg (softmax False and True), forward and backward, with the deterministic switch off and on, against the same oracle — and which
    backward entry each took: the gather entries at C = 64 either way (67200 pairs >= pointops.TRANSPOSE_MIN_PAIRS), at C = 512 the scatter entries without the
    switch and the wide gather entries with it"""
    from contrastboundary_amd import attention, neighbor_state, pointops
    assert C > 64 or n * K >= pointops.TRANSPOSE_MIN_PAIRS
    s = scene_of(n, K, C)
    tag = "%s wrappers, switch %s:" % (s.tag, "on" if switch else "off")
    d = {k: torch.from_numpy(v).cuda().requires_grad_(k not in ("g_w2", "g_out", "run_mean", "run_var")) for k, v in s.a.items()}
    idx = torch.from_numpy(s.idx).cuda()
    bn = torch.nn.BatchNorm1d(C, eps=O.EPS, momentum=O.MOMENTUM).cuda().train()
    with torch.no_grad():
        bn.running_mean.copy_(d["run_mean"]); bn.running_var.copy_(d["run_var"]); bn.num_batches_tracked.fill_(O.COUNT0)
    assert not neighbor_state.is_deterministic()
    counted.clear()
    with neighbor_state.deterministic(switch):
        w2 = attention.AttnW2.apply(d["x_q"], d["x_k"], d["p1"], d["W3C"], d["b3C"], d["gamma"], d["beta"], d["Wa"], d["ba"], idx, bn, True)
        (w2 * d["g_w2"]).sum().backward()
        torch.cuda.synchronize()
        for k, v in (("w2", w2), ("run_mean", bn.running_mean), ("run_var", bn.running_var)):
            O.close(v.detach().cpu().numpy(), s.w2[k], "%s %s" % (tag, k))
        assert int(bn.num_batches_tracked) == O.COUNT0 + 1
        O.check_w2_backward({k: d[src].grad.cpu().numpy() for k, src in O.W2_GRADS.items()}, s.w2, tag + " w2 backward", C <= 64 or switch)
        for softmax in (False, True):
            for k in ("x_v", "p1", "W3C", "b3C", "weights", "logits"):
                d[k].grad = None
            out = attention.AttnAgg.apply(d["x_v"], d["p1"], d["W3C"], d["b3C"], d["logits" if softmax else "weights"], idx, softmax)
            (out * d["g_out"]).sum().backward()
            torch.cuda.synchronize()
            ref = s.agg[int(softmax)]
            O.close(out.detach().cpu().numpy(), ref["out"], "%s agg softmax %d out" % (tag, softmax))
            grads = {k: d[src or ("logits" if softmax else "weights")].grad.cpu().numpy() for k, src in O.AGG_GRADS.items()}
            O.check_agg_backward(grads, ref, "%s agg backward softmax %d" % (tag, softmax), C <= 64 or switch, softmax, s.a["g_out"])
    assert not neighbor_state.is_deterministic()
    neighbor_state.release_unowned_transposes()
    if C <= 64:
        want = {"cbl_attn_w2_backward_csr": 1, "cbl_attn_agg_backward_csr": 2}
    elif switch:
        want = {"cbl_attn_w2_backward_wide_csr": 1, "cbl_attn_agg_backward_wide_csr": 2}
    else:
        want = {"cbl_attn_w2_backward": 1, "cbl_attn_agg_backward": 1, "cbl_attn_agg_softmax_backward": 1}
    assert {k: v for k, v in counted.items() if k in BACKWARD_ENTRIES} == want, counted
