"""CPU: the deterministic backward passes of the wide attention stages (C = 128 / 256 / 512) — `cbl_attn_w2_backward_wide_csr`, `cbl_attn_agg_backward_wide_csr`
(contrastboundary_amd/csrc/attention.hip) and `cbl_pt_layer_wide_backward_csr` (csrc/pt_layer.hip): d x_k / d x_v as gathers over the transposed neighbour
table instead of float atomics — compiled for the HOST and run with wave semantics (tests/host_emul/wave), against float64 autograd of the formulas
(tests/test_attention_host.py, tests/test_pt_layer_host.py::reference) and against the scatter entries they replace.  The transposed table is built here in
numpy, independent of neighbor_transpose.hip.  Every neighbour table holds a target no pair lists, a hub listed by more than 3 K pairs (a count that is no
multiple of 4, the gathers' unroll) and a row that lists one point K times."""
import ctypes

import numpy as np
import pytest
import torch

from tests.host_emul.host_build import P, aligned
from tests.test_attention_host import close
from tests.test_pt_layer_host import EPS, PARAMS, make, reference, rel
from tests.test_pt_layer_wide_host import host  # noqa: F401  (the fixture that builds and loads the host library)

F = ctypes.c_float

SHAPES = [(40, 16, 128), (35, 8, 128), (23, 16, 256), (17, 16, 512), (29, 5, 128)]     # the last: a ragged K against the 16-pair tile
HUB, REPEATED, REPEATED_ROW = 2, 7, lambda n: n // 3                                    # the unlisted target is n - 1


def neighbours(n, K, rng):
    """(n, K) int32: self in column 0, random elsewhere; target n - 1 listed by nobody, HUB listed by > 3 K pairs (count % 4 != 0), one row all REPEATED"""
    idx = rng.integers(0, n - 1, (n, K)).astype(np.int32)             # n - 1 never drawn
    idx[:n - 1, 0] = np.arange(n - 1)
    idx[REPEATED_ROW(n)] = REPEATED
    want = 3 * K + 1 + ((3 * K + 1) % 4 == 0)
    flat = idx.reshape(-1)
    free = np.array([p for p in range(n * K) if flat[p] != HUB and p // K != REPEATED_ROW(n) and p % K != 0])
    have = int((flat == HUB).sum())
    extra = max(want - have, 0)
    extra += (have + extra) % 4 == 0
    flat[rng.choice(free, extra, replace=False)] = HUB
    count = np.bincount(flat, minlength=n)
    assert count[n - 1] == 0 and count[HUB] >= 3 * K and count[HUB] % 4 != 0 and (idx[REPEATED_ROW(n)] == REPEATED).all()
    return idx


def transposed(idx, order):
    """segment r of inv_src: ascending, the flat pairs p = i * K + k with idx[p] == (order[r] if an order is given else r)"""
    n = idx.shape[0]
    flat = idx.reshape(-1)
    by_target = np.argsort(flat, kind="stable").astype(np.int32)
    first = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n))])
    ranks = np.arange(n) if order is None else order
    segs = [by_target[first[j]:first[j + 1]] for j in ranks]
    inv_start = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int32)
    return inv_start, np.concatenate(segs).astype(np.int32)


def case(n, K, ordered, seed):
    rng = np.random.default_rng(seed)
    idx = neighbours(n, K, rng)
    order = rng.permutation(n).astype(np.int32) if ordered else None
    return idx, order, transposed(idx, order)


def scene(n, K, C, rng):
    G = C // 8
    a = dict(x_q=rng.normal(size=(n, C)), x_k=rng.normal(size=(n, C)), x_v=rng.normal(size=(n, C)), p1=np.abs(rng.normal(size=(n, K, 3))),
             W3C=rng.normal(size=(C, 3)) * 0.5, b3C=rng.normal(size=C) * 0.1, gamma=rng.uniform(0.5, 1.5, C), beta=rng.normal(size=C) * 0.1,
             Wa=rng.normal(size=(G, C)) / np.sqrt(C), ba=rng.normal(size=G) * 0.1, logits=rng.normal(size=(n, K, G)),
             g_w2=rng.normal(size=(n, K, G)), g_out=rng.normal(size=(n, C)))
    return {k: aligned(v.astype(np.float32)) for k, v in a.items()}


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("n,K,C", SHAPES)
def test_logits_pass_gathers_d_xk(host, n, K, C, ordered):
    G, eps = C // 8, 1e-5
    idx, order, (inv_start, inv_src) = case(n, K, ordered, seed=C + K + n)
    a = scene(n, K, C, np.random.default_rng(n + C))
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in a.items()}
    ti = torch.from_numpy(idx.astype(np.int64))
    pre = t["x_k"][ti] - t["x_q"][:, None, :] + (t["p1"] @ t["W3C"].T + t["b3C"])
    flat = pre.reshape(-1, C)
    h = torch.relu((pre - flat.mean(0)) / torch.sqrt(flat.var(0, unbiased=False) + eps) * t["gamma"] + t["beta"])
    ((h @ t["Wa"].T + t["ba"]) * t["g_w2"].detach()).sum().backward()
    nbytes = host.cbl_attn_workspace_bytes(C, G)
    ws = aligned(np.zeros(nbytes // 4 + 16, np.float32))
    save_mean, save_invstd, w2 = aligned(np.zeros(C, np.float32)), aligned(np.zeros(C, np.float32)), aligned(np.zeros((n, K, G), np.float32))
    rc = host.cbl_attn_w2_forward(n, K, C, G, P(a["x_q"]), P(a["x_k"]), P(idx), P(a["p1"]), P(a["W3C"]), P(a["b3C"]), P(a["gamma"]), P(a["beta"]), F(eps), F(0.1),
                                  None, None, None, 1, P(a["Wa"]), P(a["ba"]), P(save_mean), P(save_invstd), P(w2), P(ws), ctypes.c_size_t(nbytes), None)
    assert rc == 0
    refs = dict(xq=t["x_q"].grad, xk=t["x_k"].grad, p1=t["p1"].grad, W3C=t["W3C"].grad, b3C=t["b3C"].grad, gamma=t["gamma"].grad, beta=t["beta"].grad,
                Wa=t["Wa"].grad, ba=t["ba"].grad)
    shapes = dict(xq=(n, C), xk=(n, C), p1=(n, K, 3), W3C=(C, 3), b3C=(C,), gamma=(C,), beta=(C,), Wa=(G, C), ba=(G,))
    g = {k: aligned(np.full(s, np.nan, np.float32)) for k, s in shapes.items()}
    rc = host.cbl_attn_w2_backward_wide_csr(n, K, C, G, P(a["x_q"]), P(a["x_k"]), P(idx), P(a["p1"]), P(a["W3C"]), P(a["b3C"]), P(a["gamma"]), P(a["beta"]),
                                            P(save_mean), P(save_invstd), P(a["Wa"]), P(a["g_w2"]), P(order), P(inv_start), P(inv_src),
                                            P(g["xq"]), P(g["xk"]), P(g["p1"]), P(g["W3C"]), P(g["b3C"]), P(g["gamma"]), P(g["beta"]), P(g["Wa"]), P(g["ba"]),
                                            P(ws), ctypes.c_size_t(nbytes), None)
    assert rc == 0
    assert np.isfinite(g["xk"]).all() and (g["xk"][n - 1] == 0.0).all()     # written everywhere over the NaN fill; the unlisted target exactly 0
    for k in shapes:
        if k == "b3C":                                                 # a bias in front of a train-mode BatchNorm has no gradient: what is left is rounding
            assert float(np.abs(g[k]).max()) < 1e-4 * float(refs["W3C"].abs().max())
        else:
            close(g[k], refs[k].numpy())


@pytest.mark.parametrize("softmax", [0, 1])
@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("n,K,C", SHAPES)
def test_aggregation_pass_gathers_d_xv(host, n, K, C, ordered, softmax):
    G = C // 8
    idx, order, (inv_start, inv_src) = case(n, K, ordered, seed=3 * C + K + n)
    a = scene(n, K, C, np.random.default_rng(n + 3 * C))
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in a.items()}
    ti = torch.from_numpy(idx.astype(np.int64))
    w = torch.softmax(t["logits"], 1) if softmax else t["logits"]
    out = ((t["x_v"][ti] + (t["p1"] @ t["W3C"].T + t["b3C"])) * w.repeat(1, 1, 8)).sum(1)
    (out * t["g_out"].detach()).sum().backward()
    weights = aligned(w.detach().numpy().astype(np.float32))            # softmax: the weights the forward pass keeps
    nbytes = host.cbl_attn_workspace_bytes(C, G)
    ws = aligned(np.zeros(nbytes // 4 + 16, np.float32))
    refs = dict(xv=t["x_v"].grad, p1=t["p1"].grad, W3C=t["W3C"].grad, b3C=t["b3C"].grad, a=t["logits"].grad)
    shapes = dict(xv=(n, C), p1=(n, K, 3), W3C=(C, 3), b3C=(C,), a=(n, K, G))
    g = {k: aligned(np.full(s, np.nan, np.float32)) for k, s in shapes.items()}
    rc = host.cbl_attn_agg_backward_wide_csr(n, K, C, G, P(a["x_v"]), P(idx), P(a["p1"]), P(a["W3C"]), P(a["b3C"]), P(weights), P(a["g_out"]), P(order), P(inv_start),
                                             P(inv_src), P(g["xv"]), P(g["p1"]), P(g["W3C"]), P(g["b3C"]), P(g["a"]), P(ws), ctypes.c_size_t(nbytes), softmax, None)
    assert rc == 0
    assert np.isfinite(g["xv"]).all() and (g["xv"][n - 1] == 0.0).all()
    for k in shapes:
        close(g[k], refs[k].numpy())


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("n,K,C", SHAPES)
def test_wide_layer_backward_without_atomics(host, n, K, C, ordered):
    """cbl_pt_layer_wide_backward_csr against float64 autograd (the bounds of tests/test_pt_layer_wide_host.py) and against cbl_pt_layer_wide_backward: the same
    kernels in the same order for everything but d x_k / d x_v, hence the same bits; the two gathers sum a target's pairs in another order than the host's
    sequential atomics (a few dozen fp32 terms): 1e-5 of the gradient's max."""
    idx, order, (inv_start, inv_src) = case(n, K, ordered, seed=7 * C + K + n)
    t = make(n, K, C, seed=n + C)
    t["idx"] = idx
    t = {k: aligned(v) for k, v in t.items()}
    G = C // 8
    _, grads, _, _ = reference(t, K, C)
    z = lambda *s: aligned(np.zeros(s, np.float32))
    buf = dict(p_r=z(n, K, 3), p0=z(n, K, 3), p1=z(n, K, 3), w2=z(n, K, G), a=z(n, K, G), out=z(n, C), consts=z(host.cbl_pt_layer_wide_consts_floats()), bnc=z(2 * C))
    nbytes = host.cbl_pt_layer_wide_workspace_bytes(n, K, C)
    ws = aligned(np.zeros(nbytes // 4 + 16, np.float32))
    eps3 = (F * 3)(EPS, EPS, EPS); mom3 = (F * 3)(0.1, 0.1, 0.1)
    rc = host.cbl_pt_layer_wide_forward(n, K, C, P(t["xyz"]), P(t["x_q"]), P(t["x_k"]), P(t["x_v"]), P(t["idx"]), *[P(t[k]) for k in PARAMS], eps3, mom3,
                                        None, None, None, P(buf["p_r"]), P(buf["p0"]), P(buf["p1"]), P(buf["w2"]), P(buf["a"]), P(buf["out"]), P(buf["consts"]),
                                        P(buf["bnc"]), P(ws), ctypes.c_size_t(nbytes), None)
    assert rc == 0, rc
    saved = [P(t["x_q"]), P(t["x_k"]), P(t["x_v"]), P(t["idx"])]
    rest = [P(t["gamma_p"]), P(t["W3C"]), P(t["b3C"]), P(t["gamma_c"]), P(t["beta_c"]), P(t["Wa"]), P(t["gamma_g"]), P(t["Wb"]), P(buf["p_r"]), P(buf["p0"]),
            P(buf["p1"]), P(buf["w2"]), P(buf["a"]), P(buf["consts"]), P(buf["bnc"]), P(t["g_out"])]
    fill = lambda: dict({k: aligned(np.full(t[k].shape, np.nan, np.float32)) for k in PARAMS},
                        **{k: aligned(np.full((n, C), np.nan, np.float32)) for k in ("x_q", "x_k", "x_v")})      # d x_k / d x_v not adjacent: two fills on the scatter path
    outs = lambda g: [P(g["x_q"]), P(g["x_k"]), P(g["x_v"])] + [P(g[k]) for k in PARAMS] + [P(ws), ctypes.c_size_t(nbytes), None]
    scat, gath = fill(), fill()
    assert host.cbl_pt_layer_wide_backward(n, K, C, *saved, *rest, *outs(scat)) == 0
    assert host.cbl_pt_layer_wide_backward_csr(n, K, C, *saved, P(order), P(inv_start), P(inv_src), *rest, *outs(gath)) == 0
    gmax = max(float(np.abs(v).max()) for v in grads.values())
    for k in ["x_v", "x_q", "x_k"] + PARAMS:
        assert np.isfinite(gath[k]).all(), k
        assert rel(gath[k], grads[k]) < 2e-4 or float(np.abs(gath[k] - grads[k]).max()) < 1e-5 * gmax, (k, rel(gath[k], grads[k]))
    for k in ["x_q"] + PARAMS:
        assert np.array_equal(gath[k], scat[k]), k                     # the same kernels in the same order
    for k in ("x_k", "x_v"):
        assert (gath[k][n - 1] == 0.0).all()
        assert float(np.abs(gath[k] - scat[k]).max()) < 1e-5 * float(np.abs(scat[k]).max()), k
    # without a table: an argument error, nothing launched
    assert host.cbl_pt_layer_wide_backward_csr(n, K, C, *saved, None, None, None, *rest, *outs(gath)) != 0


def test_widths_the_entries_refuse(host):
    """C = 64 through the wide entries and C = 128 through the narrow ones: non-zero (CBL_ERR_UNSUPPORTED), nothing launched; NULL tables and n = 0"""
    n, K = 20, 8
    for C, wide in ((64, True), (128, False)):
        G = C // 8
        idx, order, (inv_start, inv_src) = case(n, K, False, seed=C)
        a = scene(n, K, C, np.random.default_rng(C))
        nbytes = host.cbl_attn_workspace_bytes(C, G)
        ws = aligned(np.zeros(nbytes // 4 + 16, np.float32))
        z = lambda *s: aligned(np.zeros(s, np.float32))
        w2 = host.cbl_attn_w2_backward_wide_csr if wide else host.cbl_attn_w2_backward_csr
        agg = host.cbl_attn_agg_backward_wide_csr if wide else host.cbl_attn_agg_backward_csr
        stat = z(C) + 1
        w2_args = lambda n_, tbl: (n_, K, C, G, P(a["x_q"]), P(a["x_k"]), P(idx), P(a["p1"]), P(a["W3C"]), P(a["b3C"]), P(a["gamma"]), P(a["beta"]), P(stat), P(stat),
                                   P(a["Wa"]), P(a["g_w2"]), None, *tbl, P(z(n, C)), P(z(n, C)), P(z(n, K, 3)), P(z(C, 3)), P(z(C)), P(z(C)), P(z(C)), P(z(G, C)), P(z(G)),
                                   P(ws), ctypes.c_size_t(nbytes), None)
        agg_args = lambda n_, tbl: (n_, K, C, G, P(a["x_v"]), P(idx), P(a["p1"]), P(a["W3C"]), P(a["b3C"]), P(a["logits"]), P(a["g_out"]), None, *tbl,
                                    P(z(n, C)), P(z(n, K, 3)), P(z(C, 3)), P(z(C)), P(z(n, K, G)), P(ws), ctypes.c_size_t(nbytes), 0, None)
        assert w2(*w2_args(n, (P(inv_start), P(inv_src)))) != 0
        assert agg(*agg_args(n, (P(inv_start), P(inv_src)))) != 0
    C, G = 128, 16                                                      # (a, idx, ws of the last round: C = 128)
    assert host.cbl_attn_w2_backward_wide_csr(*w2_args(n, (None, None))) == -1 and host.cbl_attn_agg_backward_wide_csr(*agg_args(n, (None, None))) == -1
    assert host.cbl_attn_w2_backward_wide_csr(*w2_args(0, (None, None))) == 0 and host.cbl_attn_agg_backward_wide_csr(*agg_args(0, (None, None))) == 0
