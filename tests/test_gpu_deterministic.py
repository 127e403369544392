"""The deterministic training mode (neighbor_state.deterministic, re-exported by the package): with the switch on no backward pass of the Point Transformer path
adds with float atomics, so two runs from the same state give the same BITS.  The three *_wide_csr entries through ctypes against the scatter entries they
replace; a wide layer on its three routes; the generic operators below pointops.TRANSPOSE_MIN_PAIRS; a replayed hipGraph; a stage; the whole model."""
import copy
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_i, _f = ctypes.c_int, ctypes.c_float


def rel(a, b):
    return float((a.detach().double() - b.detach().double()).norm() / max(float(b.detach().double().norm()), 1e-30))


def of_max(a, b):
    return float((a.detach().double() - b.detach().double()).abs().max()) / max(float(b.detach().double().abs().max()), 1e-30)


def neighbours(n, K, seed):
    """(n, K) int32 on the device: self in column 0, random elsewhere; target n - 1 listed by nobody, target 2 by more than 3 K pairs (a count that is no multiple
    of 4), row n // 3 lists target 7 K times"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n - 1, (n, K)).astype(np.int32)
    idx[:n - 1, 0] = np.arange(n - 1)
    idx[n // 3] = 7
    flat = idx.reshape(-1)
    free = np.array([p for p in range(n * K) if flat[p] != 2 and p // K != n // 3 and p % K != 0])
    have = int((flat == 2).sum())
    extra = max(3 * K + 1 - have, 0)
    extra += (have + extra) % 4 == 0
    flat[rng.choice(free, extra, replace=False)] = 2
    count = np.bincount(flat, minlength=n)
    assert count[n - 1] == 0 and count[2] >= 3 * K and count[2] % 4 != 0 and (idx[n // 3] == 7).all()
    return torch.from_numpy(idx).cuda()


class CountingLib:
    """the ctypes library with every entry looked up on it counted by name"""

    def __init__(self, real):
        self.real, self.calls = real, {}

    def __getattr__(self, name):
        self.calls[name] = self.calls.get(name, 0) + 1
        return getattr(self.real, name)


@pytest.fixture
def counted(monkeypatch):
    from contrastboundary_amd import _lib
    proxy = CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: proxy)
    return proxy.calls


# ---------------------------------------------------------------------------------------------------------------- 1. the entries
@pytest.mark.parametrize("n,K,C", [(160, 16, 512), (97, 16, 256), (640, 16, 128), (35, 8, 128)])
def test_wide_gather_entries_against_the_scatter_entries(n, K, C):
    """d x_k / d x_v of cbl_attn_w2_backward_wide_csr / cbl_attn_agg_backward_wide_csr (softmax 0 and 1) within 1e-4 of max of the atomic entries'
    (tests/test_gpu_blocks.py's bound for these passes), every other output too; two calls give the same bits; an unlisted target gets exact zeros.
    (cbl_pt_layer_wide_backward_csr, which calls the two: through the layer, below.)"""
    from contrastboundary_amd import _lib, pointops
    L, P = _lib.lib(), _lib.ptr
    G = C // 8
    torch.manual_seed(n + C)
    idx = neighbours(n, K, n + K)
    order, inv_start, inv_src = pointops.neighbor_transpose(idx, n, build=True)
    r = lambda *s: torch.randn(*s, device="cuda")
    x_q, x_k, x_v, p1 = r(n, C), r(n, C), r(n, C), r(n, K, 3).abs()
    W3C, b3C, gamma, beta, Wa, ba = r(C, 3) * 0.5, r(C) * 0.1, torch.rand(C, device="cuda") + 0.5, r(C) * 0.1, r(G, C) / C ** 0.5, r(G) * 0.1
    g_w2, g_out, a = r(n, K, G), r(n, C), torch.softmax(r(n, K, G), 1).contiguous()
    st = _lib.stream_of(x_q)
    ws = torch.empty(L.cbl_attn_workspace_bytes(_i(C), _i(G)) + 256, dtype=torch.uint8, device="cuda")
    wsn = ctypes.c_size_t(ws.numel())
    mean, invstd, w2 = torch.empty(C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(n, K, G, device="cuda")
    _lib.check(L.cbl_attn_w2_forward(_i(n), _i(K), _i(C), _i(G), P(x_q), P(x_k), P(idx), P(p1), P(W3C), P(b3C), P(gamma), P(beta), _f(1e-5), _f(0.1), None, None, None,
                                     _i(1), P(Wa), P(ba), P(mean), P(invstd), P(w2), P(ws), wsn, st), "cbl_attn_w2_forward")
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")

    def w2_bwd(gather):
        g = dict(xq=nan(n, C), xk=nan(n, C) if gather else torch.zeros(n, C, device="cuda"), p1=nan(n, K, 3), W3C=nan(C, 3), b3C=nan(C), gamma=nan(C), beta=nan(C),
                 Wa=nan(G, C), ba=nan(G))
        head = (_i(n), _i(K), _i(C), _i(G), P(x_q), P(x_k), P(idx), P(p1), P(W3C), P(b3C), P(gamma), P(beta), P(mean), P(invstd), P(Wa), P(g_w2))
        tail = tuple(P(g[k]) for k in ("xq", "xk", "p1", "W3C", "b3C", "gamma", "beta", "Wa", "ba")) + (P(ws), wsn, st)
        if gather:
            _lib.check(L.cbl_attn_w2_backward_wide_csr(*head, P(order), P(inv_start), P(inv_src), *tail), "cbl_attn_w2_backward_wide_csr")
        else:
            _lib.check(L.cbl_attn_w2_backward(*head, *tail), "cbl_attn_w2_backward")
        return g

    def agg_bwd(gather, softmax):
        g = dict(xv=nan(n, C) if gather else torch.zeros(n, C, device="cuda"), p1=nan(n, K, 3), W3C=nan(C, 3), b3C=nan(C), a=nan(n, K, G))
        head = (_i(n), _i(K), _i(C), _i(G), P(x_v), P(idx), P(p1), P(W3C), P(b3C), P(a), P(g_out))
        tail = tuple(P(g[k]) for k in ("xv", "p1", "W3C", "b3C", "a")) + (P(ws), wsn)
        if gather:
            _lib.check(L.cbl_attn_agg_backward_wide_csr(*head, P(order), P(inv_start), P(inv_src), *tail, _i(softmax), st), "cbl_attn_agg_backward_wide_csr")
        else:
            _lib.check((L.cbl_attn_agg_softmax_backward if softmax else L.cbl_attn_agg_backward)(*head, *tail, st), "cbl_attn_agg_backward")
        return g

    for run in (w2_bwd, lambda gather: agg_bwd(gather, 0), lambda gather: agg_bwd(gather, 1)):
        scat, one, two = run(False), run(True), run(True)
        torch.cuda.synchronize()
        for k in scat:
            assert torch.isfinite(one[k]).all(), k
            assert torch.equal(one[k], two[k]), k
            if k == "b3C" and run is w2_bwd:                           # no gradient through a train-mode BatchNorm: rounding only, on both sides
                continue
            print("n %d K %d C %d %s: gather vs scatter %.2e of max" % (n, K, C, k, of_max(one[k], scat[k])))
            assert of_max(one[k], scat[k]) < 1e-4, k
        target = "xk" if "xk" in one else "xv"
        assert bool((one[target][n - 1] == 0).all())


# ---------------------------------------------------------------------------------------------------------------- 2. the layer
def _layer_run(layer, xyz, x0, o, idx, g):
    layer = copy.deepcopy(layer)
    x = x0.clone().requires_grad_(True)
    y = layer([xyz, x, o], idx)
    y.backward(g)
    torch.cuda.synchronize()
    return [y.detach(), x.grad] + [p.grad for p in layer.parameters()]


@pytest.mark.parametrize("fused", [True, "qkv3", "split"])
@pytest.mark.parametrize("n,C", [(160, 512), (640, 128)])
def test_wide_layer_gives_the_same_bits_twice(counted, n, C, fused):
    import contrastboundary_amd
    from contrastboundary_amd import blocks, pointops, synthetic as S
    torch.manual_seed(n + C)
    xyz = torch.from_numpy(S.s_room(n, seed=3)[0]).cuda()
    o = torch.tensor([n], dtype=torch.int32, device="cuda")
    idx = pointops.knn_indices(16, xyz, xyz, o, o)
    layer = blocks.PointTransformerLayer(C, C, 8, 16).cuda().train()
    layer.fused = fused
    x, g = torch.randn(n, C, device="cuda"), torch.randn(n, C, device="cuda")
    off = _layer_run(layer, xyz, x, o, idx, g)
    assert not contrastboundary_amd.is_deterministic()
    counted.clear()
    with contrastboundary_amd.deterministic():
        one = _layer_run(layer, xyz, x, o, idx, g)
        two = _layer_run(layer, xyz, x, o, idx, g)
    assert not contrastboundary_amd.is_deterministic()
    if fused is True:
        assert "cbl_pt_layer_wide_backward" not in counted and counted.get("cbl_pt_layer_wide_backward_csr") == 2, counted
    elif fused == "split":
        assert counted.get("cbl_attn_w2_backward_wide_csr") == 2 and counted.get("cbl_attn_agg_backward_wide_csr") == 2, counted
        assert not {"cbl_attn_w2_backward", "cbl_attn_agg_softmax_backward", "cbl_attn_agg_backward", "cbl_grouping_backward"} & set(counted), counted
    names = ["y", "grad_x"] + [k for k, _ in layer.named_parameters()]
    for k, a, b in zip(names, one, two):
        assert torch.equal(a, b), k
    # against the default path: the bounds of tests/test_gpu_blocks.py::test_wide_layer_one_call_equals_ops
    assert rel(one[0], off[0]) < 2e-5 and rel(one[1], off[1]) < 2e-4
    gmax = max(float(t.abs().max()) for t in off[2:])
    for k, a, b in zip(names[2:], one[2:], off[2:]):
        assert rel(a, b) < 5e-4 or float((a - b).abs().max()) < 1e-4 * gmax, k


def test_the_switch_is_process_global_and_off_by_default():
    import contrastboundary_amd
    from contrastboundary_amd import neighbor_state
    assert contrastboundary_amd.deterministic is neighbor_state.deterministic and contrastboundary_amd.set_deterministic is neighbor_state.set_deterministic
    assert not neighbor_state.is_deterministic()
    with neighbor_state.deterministic():
        seen = []
        import threading
        t = threading.Thread(target=lambda: seen.append(neighbor_state.is_deterministic()))
        t.start(); t.join()
        assert seen == [True]                                           # autograd's thread sees it
        with neighbor_state.deterministic(False):
            assert not neighbor_state.is_deterministic()
        assert neighbor_state.is_deterministic()
    assert not neighbor_state.is_deterministic()


# ---------------------------------------------------------------------------------------------------------------- 3. the generic operators
def _generic(name, m, K, C):
    """-> (function of nothing returning the gradients of one forward + backward, csr entry, atomic entry or None)"""
    from contrastboundary_amd import pointops, synthetic as S
    torch.manual_seed(m)
    xyz = torch.from_numpy(S.s_room(m, seed=4)[0]).cuda()
    o = torch.tensor([m], dtype=torch.int32, device="cuda")
    r = lambda *s: torch.randn(*s, device="cuda")
    if name == "queryandgroup":
        feat, g = r(m, C), r(m, K, 3 + C)

        def run():
            f = feat.clone().requires_grad_(True)
            pointops.queryandgroup(K, xyz, xyz, f, None, o, o, use_xyz=True).backward(g)
            return [f.grad]
        return run, "cbl_grouping_backward_csr_rows", "cbl_grouping_backward"
    if name == "interpolation":
        coarse = xyz[::4].contiguous()
        oc = torch.tensor([coarse.shape[0]], dtype=torch.int32, device="cuda")
        feat, g = r(coarse.shape[0], C), r(m, C)

        def run():
            f = feat.clone().requires_grad_(True)
            pointops.interpolation(coarse, xyz, f, oc, o).backward(g)
            return [f.grad]
        return run, "cbl_weighted_scatter_csr", "cbl_interpolation_backward"
    idx = pointops.knn_indices(K, xyz, xyz, o, o)
    if name == "weighted_gather":
        feat, w, g = r(m, C), torch.rand(m, K, device="cuda"), r(m, C)

        def run():
            f = feat.clone().requires_grad_(True)
            pointops.WeightedGather.apply(f, idx, w).backward(g)
            return [f.grad]
        return run, "cbl_weighted_scatter_csr", "cbl_interpolation_backward"
    if name == "subtraction":
        a, b, g = r(m, C), r(m, C), r(m, K, C)

        def run():
            ta, tb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
            pointops.subtraction(ta, tb, idx).backward(g)
            return [ta.grad, tb.grad]
        return run, "cbl_subtraction_backward_csr", "cbl_subtraction_backward"
    x, pos, w, g = r(m, C), r(m, K, C), r(m, K, C // 8), r(m, C)

    def run():
        tx, tp, tw = x.clone().requires_grad_(True), pos.clone().requires_grad_(True), w.clone().requires_grad_(True)
        pointops.aggregation(tx, tp, tw, idx).backward(g)
        return [tx.grad, tp.grad, tw.grad]
    return run, "cbl_weighted_scatter_csr", None                        # (K10 runs in both modes, without its grad_input under the switch)


@pytest.mark.parametrize("name", ["queryandgroup", "interpolation", "subtraction", "aggregation", "weighted_gather"])
def test_generic_operators_build_their_table_under_the_switch(counted, name):
    from contrastboundary_amd import neighbor_state, pointops
    m, K, C = 200, 16, 32
    assert m * K < pointops.TRANSPOSE_MIN_PAIRS // 8
    run, csr, atomic = _generic(name, m, K, C)
    counted.clear()
    off = run()
    assert csr not in counted and (atomic is None or counted.get(atomic)), counted
    neighbor_state.release_unowned_transposes()
    counted.clear()
    with neighbor_state.deterministic():
        one = run()
        two = run()
    torch.cuda.synchronize()
    neighbor_state.release_unowned_transposes()
    assert counted.get(csr) and (atomic is None or atomic not in counted), counted
    for a, b, c in zip(one, two, off):
        assert torch.equal(a, b)
        assert of_max(a, c) < 1e-5, of_max(a, c)


# ---------------------------------------------------------------------------------------------------------------- 4. a replayed graph
def test_wide_layer_in_a_replayed_graph_under_the_switch():
    from contrastboundary_amd import blocks, neighbor_state, pointops, synthetic as S
    n, C = 160, 256
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
    with neighbor_state.deterministic():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        neighbor_state.release_unowned_transposes()                     # the warm-up's table: the capture builds its own (as a captured training step does)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step()
    neighbor_state.release_unowned_transposes()                         # ... which lives in the graph's pool: the eager run below builds another
    nx, ng = torch.randn(n, C, device="cuda"), torch.randn(n, C, device="cuda")
    with torch.no_grad():
        x.copy_(nx); g.copy_(ng)
    graph.replay()                                                      # the switch is off again: the graph holds the gather kernels
    torch.cuda.synchronize()
    first = [t.clone() for t in out]
    graph.replay()
    torch.cuda.synchronize()
    with neighbor_state.deterministic():
        ex = nx.clone().requires_grad_(True)
        y = eager_layer([xyz, ex, o], idx)
        eager = [y.detach()] + list(torch.autograd.grad(y, [ex] + list(eager_layer.parameters()), ng))
    for k, a, b, c in zip(["y", "grad_x"] + [k for k, _ in layer.named_parameters()], first, out, eager):
        assert torch.equal(a, b), k
        assert torch.equal(a, c), k


# ---------------------------------------------------------------------------------------------------------------- 5. a stage
def test_a_wide_stage_gives_the_same_bits_twice():
    from contrastboundary_amd import blocks, neighbor_state, synthetic as S
    n = 640
    torch.manual_seed(5)
    xyz = torch.from_numpy(S.s_room(n, seed=6)[0]).cuda()
    o = torch.tensor([n], dtype=torch.int32, device="cuda")
    x = torch.randn(n, 64, device="cuda")
    stage = torch.nn.Sequential(blocks.TransitionDown(64, 128, 4, 16), blocks.PointTransformerBlock(128, 128, 8, 16), blocks.PointTransformerBlock(128, 128, 8, 16)).cuda().train()

    def run():
        twin = copy.deepcopy(stage)
        xin = x.clone().requires_grad_(True)
        p, y, _ = twin([xyz, xin, o])
        assert p.shape[0] == n // 4
        (y * y).sum().backward()
        torch.cuda.synchronize()
        return {"x": xin.grad, **{k: v.grad for k, v in twin.named_parameters()}}
    with neighbor_state.deterministic():
        one, two = run(), run()
    assert all(v is not None for v in one.values())
    for k in one:
        assert torch.equal(one[k], two[k]), k


# ---------------------------------------------------------------------------------------------------------------- 6. the model
def test_two_eager_trajectories_of_the_model_are_equal():
    """two 2-step SGD trajectories from deep copies of the model (as tools/traj_determinism.py runs them), under the switch: the same losses and parameters,
    bit for bit"""
    from contrastboundary_amd import neighbor_state
    from tests.test_gpu_model import CASES, build
    M, model, crit, g = build(CASES[0])
    model = model.cuda().train()
    inputs = {"points": torch.from_numpy(g("xyz")).cuda(), "features": torch.from_numpy(g("feat")).cuda(), "offset": torch.from_numpy(g("offset")).cuda()}
    target = torch.from_numpy(g("target")).cuda()
    inputs2 = {"points": (inputs["points"] * torch.tensor([-1.0, 1.0, 1.0], device="cuda")).contiguous(), "features": inputs["features"].flip(0).contiguous(),
               "offset": inputs["offset"].clone()}
    batches = [(inputs, target), (inputs2, target.roll(17))]
    runs = []
    with neighbor_state.deterministic():
        for r in range(2):
            twin = copy.deepcopy(model)
            opt = torch.optim.SGD(twin.parameters(), lr=0.002, momentum=0.9)
            losses = []
            for b_in, b_tg in batches:
                opt.zero_grad(set_to_none=True)
                _, _, loss, _ = M.forward_and_loss(twin, crit, b_in, b_tg)
                loss.sum().backward()
                opt.step()
                losses.append(loss.detach().clone())
                neighbor_state.release_unowned_transposes()
            torch.cuda.synchronize()
            runs.append((losses, {k: v.detach().clone() for k, v in twin.state_dict().items()}))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b), (a, b)
    differ = [k for k in runs[0][1] if not torch.equal(runs[0][1][k], runs[1][1][k])]
    assert not differ, differ[:8]
