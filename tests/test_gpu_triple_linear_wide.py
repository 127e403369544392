"""The q / k / v projections of the wide attention stages (C = 128 | 256 | 512) on the library's own kernels (cbl_triple_linear_*, csrc/skinny_linear.hip):
`dense.triple_linear` against F.linear in float64 at the stage shapes, no library GEMM on the training path of a wide layer, the same bits whether or not the
three weights are adjacent, from call to call and from a replayed hipGraph, evaluation mode, and the C entry points through ctypes."""
import copy
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

STAGES = [(2560, 128), (640, 256), (160, 512)]                       # (points, width) of the three wide stages, one scene
SHAPES = [(s * n, C) for n, C in STAGES for s in (1, 4, 8)] + [(2563, 128), (777, 256), (161, 512)]


def rel(a, b):
    return float((a.detach().double() - b.detach().double()).norm() / max(float(b.detach().double().norm()), 1e-30))


def projections(C, seed):
    torch.manual_seed(seed)
    return [nn.Linear(C, C).cuda() for _ in range(3)]


def run_triple(x, ls, gs):
    """dense.triple_linear forward + backward: (q, k, v, grad_x, 3 weight gradients, 3 bias gradients)"""
    from contrastboundary_amd import dense
    params = [l.weight for l in ls] + [l.bias for l in ls]
    ys = dense.triple_linear(x, *ls)
    grads = torch.autograd.grad(ys, [x] + params, gs)
    return [y.detach() for y in ys] + list(grads)


@pytest.mark.parametrize("rows,C", SHAPES)
def test_triple_linear_against_float64(rows, C):
    """bounds of tests/test_gpu_dense.py::test_triple_linear_equals_three_linear_layers: relative L2 error below 1e-6 for y and grad_x, below 1e-5 for the
    weight and bias gradients (the fp32 MFMA chain sits at 1e-7 .. 6e-7 on these in a numpy model of it)"""
    ls = projections(C, rows + C)
    x = torch.randn(rows, C, device="cuda", requires_grad=True)
    gs = [torch.randn(rows, C, device="cuda") for _ in range(3)]
    got = run_triple(x, ls, gs)
    x64 = x.detach().double().requires_grad_(True)
    ws = [l.weight.detach().double().requires_grad_(True) for l in ls]
    bs = [l.bias.detach().double().requires_grad_(True) for l in ls]
    ys64 = [F.linear(x64, w, b) for w, b in zip(ws, bs)]
    torch.autograd.backward(ys64, [g.double() for g in gs])
    figures = [rel(y, y64) for y, y64 in zip(got[:3], ys64)] + [rel(got[3], x64.grad)] + [rel(g, w.grad) for g, w in zip(got[4:7], ws)] + \
              [rel(g, b.grad) for g, b in zip(got[7:10], bs)]
    print("rows %d C %d: y %.2e %.2e %.2e, grad_x %.2e, grad_w %.2e %.2e %.2e, grad_b %.2e %.2e %.2e" % (rows, C, *figures))
    assert all(f < 1e-6 for f in figures[:4]), figures
    assert all(f < 1e-5 for f in figures[4:]), figures


def _no_library_gemm(monkeypatch):
    def refuse(name):
        def f(*a, **k):
            raise AssertionError("a library GEMM (%s) on the path of the wide projections" % name)
        return f
    for name in ("baddbmm", "bmm", "matmul", "addmm"):
        monkeypatch.setattr(torch, name, refuse("torch." + name))
    monkeypatch.setattr(torch.nn.functional, "linear", refuse("torch.nn.functional.linear"))


@pytest.mark.parametrize("n,C", STAGES)
def test_no_library_gemm_on_the_path(monkeypatch, n, C):
    """a training forward + backward of a wide layer, and dense.triple_linear under no_grad (what an evaluation-mode layer calls), complete with torch's GEMM
    entry points replaced by functions that raise"""
    from contrastboundary_amd import blocks, dense, pointops, synthetic as S
    torch.manual_seed(n)
    xyz = torch.from_numpy(S.s_room(n, seed=2)[0]).cuda()
    o = torch.tensor([n], dtype=torch.int32, device="cuda")
    layer = blocks.PointTransformerLayer(C, C, 8, 16).cuda().train()
    idx = pointops.knn_indices(16, xyz, xyz, o, o)
    x = torch.randn(n, C, device="cuda", requires_grad=True)
    g = torch.randn(n, C, device="cuda")
    _no_library_gemm(monkeypatch)
    y = layer([xyz, x, o], idx)
    y.backward(g)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in layer.parameters())
    with torch.no_grad():
        q, k, v = dense.triple_linear(x.detach(), layer.linear_q, layer.linear_k, layer.linear_v)
    torch.cuda.synchronize()
    monkeypatch.undo()
    for out, l in zip((q, k, v), (layer.linear_q, layer.linear_k, layer.linear_v)):
        assert rel(out, F.linear(x.detach().double(), l.weight.detach().double(), l.bias.detach().double())) < 1e-6


@pytest.mark.parametrize("n,C", STAGES)
def test_adjacent_and_separate_weights_give_the_same_bits(n, C):
    """the entries take the three weights by pointer: after pt_layer.adjoin_qkv (one storage, back to back) q, k, v and every gradient of dense.triple_linear
    are bit-identical to those with freshly allocated weights.  The whole layer is compared within the bounds of
    tests/test_gpu_blocks.py::test_wide_layer_with_adjacent_projections only: its backward adds d x_k and d x_v with float atomics, so the layer's forward
    alone is bit-reproducible."""
    from contrastboundary_amd import blocks, pointops, pt_layer, synthetic as S
    torch.manual_seed(11 * C + n)
    xyz = torch.from_numpy(S.s_room(n, seed=5)[0]).cuda()
    o = torch.tensor([n], dtype=torch.int32, device="cuda")
    idx = pointops.knn_indices(16, xyz, xyz, o, o)
    layer = blocks.PointTransformerLayer(C, C, 8, 16).cuda().train()
    sep = copy.deepcopy(layer)
    pt_layer.adjoin_qkv(layer)
    trip = lambda m: (m.linear_q, m.linear_k, m.linear_v)
    assert pt_layer._adjacent([l.weight.data for l in trip(layer)]) and not pt_layer._adjacent([l.weight.data for l in trip(sep)])
    x = torch.randn(n, C, device="cuda", requires_grad=True)
    gs = [torch.randn(n, C, device="cuda") for _ in range(3)]
    for a, b in zip(run_triple(x, trip(layer), gs), run_triple(x, trip(sep), gs)):
        assert torch.equal(a, b)
    g = torch.randn(n, C, device="cuda")
    x1 = x.detach().clone().requires_grad_(True); x2 = x.detach().clone().requires_grad_(True)
    y1 = layer([xyz, x1, o], idx); y1.backward(g)
    y2 = sep([xyz, x2, o], idx); y2.backward(g)
    assert torch.equal(y1, y2)
    assert rel(x1.grad, x2.grad) < 2e-4
    gmax = max(float(pb.grad.abs().max()) for pb in sep.parameters())
    for (name, pa), (_, pb) in zip(layer.named_parameters(), sep.named_parameters()):
        assert pa.grad is not None and (rel(pa.grad, pb.grad) < 5e-4 or float((pa.grad - pb.grad).abs().max()) < 1e-4 * gmax), name


@pytest.mark.parametrize("rows,C", STAGES + [(20480, 128), (5120, 256), (1280, 512)])
def test_two_runs_give_identical_bits(rows, C):
    ls = projections(C, 3 * rows + C)
    x = torch.randn(rows, C, device="cuda", requires_grad=True)
    gs = [torch.randn(rows, C, device="cuda") for _ in range(3)]
    first = [t.clone() for t in run_triple(x, ls, gs)]
    torch.empty(1 << 22, device="cuda").normal_()                    # other work in between: the second run's outputs land in other memory
    for a, b in zip(first, run_triple(x, ls, gs)):
        assert torch.equal(a, b)


def _capture(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    return graph, out


@pytest.mark.parametrize("rows,C", [(640, 256)])
def test_triple_linear_in_a_replayed_graph(rows, C):
    """forward + backward of dense.triple_linear captured once (no allocation or synchronisation inside the entries), replayed three times on new inputs copied
    into the captured tensors: equal to the eager call bit for bit"""
    ls = projections(C, 5)
    x = torch.randn(rows, C, device="cuda", requires_grad=True)
    gs = [torch.randn(rows, C, device="cuda") for _ in range(3)]
    graph, out = _capture(lambda: run_triple(x, ls, gs))
    for trial in range(3):
        nx = torch.randn(rows, C, device="cuda"); ngs = [torch.randn(rows, C, device="cuda") for _ in range(3)]
        with torch.no_grad():
            x.copy_(nx)
            for g, ng in zip(gs, ngs):
                g.copy_(ng)
        graph.replay()
        torch.cuda.synchronize()
        eager = run_triple(nx.clone().requires_grad_(True), ls, ngs)
        for a, b in zip(out, eager):
            assert torch.equal(a, b), trial


@pytest.mark.parametrize("n,C", [(640, 256)])
def test_wide_layer_in_a_replayed_graph(n, C):
    """one whole wide layer (projections included), captured and replayed on new inputs, against the eager layer within the bounds of
    tests/test_gpu_blocks.py::test_wide_layer_one_call_equals_ops (the layer's backward uses float atomics: not bit-reproducible)"""
    from contrastboundary_amd import blocks, pointops, synthetic as S
    torch.manual_seed(n + C)
    xyz = torch.from_numpy(S.s_room(n, seed=3)[0]).cuda()
    o = torch.tensor([n], dtype=torch.int32, device="cuda")
    idx = pointops.knn_indices(16, xyz, xyz, o, o)
    layer = blocks.PointTransformerLayer(C, C, 8, 16).cuda().train()
    eager_layer = copy.deepcopy(layer)
    params = list(layer.parameters())
    x = torch.randn(n, C, device="cuda", requires_grad=True)
    g = torch.randn(n, C, device="cuda")

    def step():
        y = layer([xyz, x, o], idx)
        return [y.detach()] + list(torch.autograd.grad(y, [x] + params, g))
    graph, out = _capture(step)
    for trial in range(3):
        nx, ng = torch.randn(n, C, device="cuda"), torch.randn(n, C, device="cuda")
        with torch.no_grad():
            x.copy_(nx); g.copy_(ng)
        graph.replay()
        torch.cuda.synchronize()
        ex = nx.clone().requires_grad_(True)
        y = eager_layer([xyz, ex, o], idx)
        grads = torch.autograd.grad(y, [ex] + list(eager_layer.parameters()), ng)
        gmax = max(float(t.abs().max()) for t in grads[1:])
        figures = {name: (rel(a, b), float((a - b).abs().max()) / gmax) for (name, _), a, b in zip(layer.named_parameters(), out[2:], grads[1:])}
        print("trial %d: y %.2e, grad_x %.2e, parameters (relative L2, largest difference / largest gradient) %s"
              % (trial, rel(out[0], y), rel(out[1], grads[0]), {k: "%.1e %.1e" % v for k, v in figures.items()}))
        assert rel(out[0], y) < 2e-5 and rel(out[1], grads[0]) < 2e-4, trial
        for name, (r, d) in figures.items():
            assert r < 5e-4 or d < 1e-4, (trial, name)


@pytest.mark.parametrize("n,C", STAGES)
def test_eval_mode_layer_equals_three_library_projections(monkeypatch, n, C):
    """a wide layer in eval() under no_grad — its projections now on cbl_triple_linear_forward — against the same call with dense.triple_linear replaced by
    three F.linear calls: output within 1e-4 of the largest element (the bound tests/test_gpu_blocks.py uses for a layer output)"""
    from contrastboundary_amd import blocks, dense, pointops, synthetic as S
    torch.manual_seed(n + 2 * C)
    xyz = torch.from_numpy(S.s_room(n, seed=4)[0]).cuda()
    o = torch.tensor([n], dtype=torch.int32, device="cuda")
    idx = pointops.knn_indices(16, xyz, xyz, o, o)
    layer = blocks.PointTransformerLayer(C, C, 8, 16).cuda()
    x = torch.randn(n, C, device="cuda")
    with torch.no_grad():
        layer.train()
        layer([xyz, x, o], idx)                                      # running statistics away from their initial values
        layer.eval()
        ours = layer([xyz, x, o], idx)
        calls = []
        monkeypatch.setattr(dense, "triple_linear", lambda t, lq, lk, lv: (calls.append(1), (F.linear(t, lq.weight, lq.bias), F.linear(t, lk.weight, lk.bias),
                                                                                             F.linear(t, lv.weight, lv.bias)))[1])
        ref = layer([xyz, x, o], idx)
    assert calls
    err = float((ours.double() - ref.double()).abs().max()) / float(ref.double().abs().max())
    print("n %d C %d: eval output, largest difference / largest element %.2e" % (n, C, err))
    assert err < 1e-4


@pytest.mark.parametrize("C", [128, 256, 512])
@pytest.mark.parametrize("rows", [1, 17])
@pytest.mark.parametrize("null_bias,grad_bias", [(None, "all"), (1, "none"), (0, 2)])
def test_entries_through_the_c_abi(rows, C, null_bias, grad_bias):
    """cbl_triple_linear_forward / _backward by ctypes on raw device pointers: one row, one row past a tile, bias3 / grad_bias3 entries (or the array) NULL;
    outputs pre-filled with NaN, a red zone behind a workspace of exactly cbl_triple_linear_workspace_bytes(C)"""
    from contrastboundary_amd import _lib
    L = _lib.lib()
    torch.manual_seed(rows + C)
    dev = "cuda"
    x = torch.randn(rows, C, device=dev)
    W = [torch.randn(C, C, device=dev) / C ** 0.5 for _ in range(3)]
    b = [torch.randn(C, device=dev) for _ in range(3)]
    gy = [torch.randn(rows, C, device=dev) for _ in range(3)]
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    y, gx, gW = [nan(rows, C) for _ in range(3)], nan(rows, C), [nan(C, C) for _ in range(3)]
    gb = [None if grad_bias in ("none", p) else nan(C) for p in range(3)]
    arr = lambda ts: (ctypes.c_void_p * 3)(*[None if t is None else t.data_ptr() for t in ts])
    b_in = [None if p == null_bias else b[p] for p in range(3)]
    st = _lib.stream_of(x)
    assert L.cbl_triple_linear_forward(ctypes.c_longlong(rows), ctypes.c_int(C), _lib.ptr(x), arr(W), arr(b_in), arr(y), st) == 0
    nbytes = L.cbl_triple_linear_workspace_bytes(ctypes.c_int(C))
    ws = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    assert L.cbl_triple_linear_backward(ctypes.c_longlong(rows), ctypes.c_int(C), _lib.ptr(x), arr(W), arr(gy), _lib.ptr(gx), arr(gW),
                                        None if grad_bias == "none" else arr(gb), _lib.ptr(ws), ctypes.c_size_t(nbytes), st) == 0
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all())
    x64 = x.double()
    for p in range(3):
        assert rel(y[p], x64 @ W[p].double().t() + (0 if b_in[p] is None else b[p].double())) < 1e-6
        assert rel(gW[p], gy[p].double().t() @ x64) < 1e-5
        if gb[p] is not None:
            assert rel(gb[p], gy[p].double().sum(0)) < 1e-5
    assert rel(gx, sum(gy[p].double() @ W[p].double() for p in range(3))) < 1e-6
    assert L.cbl_triple_linear_forward(ctypes.c_longlong(rows), ctypes.c_int(96), _lib.ptr(x), arr(W), arr(b), arr(y), st) == -3
    assert L.cbl_triple_linear_backward(ctypes.c_longlong(rows), ctypes.c_int(C), _lib.ptr(x), arr(W), arr(gy), _lib.ptr(gx), arr(gW), None, _lib.ptr(ws),
                                        ctypes.c_size_t(nbytes - 1), st) == -2
