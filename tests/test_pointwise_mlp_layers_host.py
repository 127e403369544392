"""CPU: the PointWiseMLP kernels for fc_num 2 and 3 (contrastboundary_amd/csrc/pointwise_mlp_layers.hip; tensorflow/models/local_aggregation_operators.py:503-617
with the layers of :589-600) compiled for the HOST and run with wave semantics (tests/host_emul/wave: the MFMA chain is emulated in its own lane layout),
through their C entry points, against the float64 restatement of the graph code in its direct form (tests/pointwise_mlp_layers_oracle.py) within the 1e-4
contract.  The fold of the first layer into per-point terms and the chain back to the features and the first layer's weights are done here in numpy, as the
Python mirror leaves them to autograd.  The workspace is poisoned with 0xff and every output with NaN before each call.  Gradient cases with an activation or
'max' assert, from the oracle, that no relu or arg-max can flip between fp32 and float64 (seeds chosen so).
A stand-alone AddressSanitizer program (tests/host_emul/pointwise_mlp_layers_asan_main.cpp) runs the same translation unit over the shape edges with heap
buffers of exactly their logical size: an indexing error of a kernel surfaces there, on the CPU."""
import ctypes

import numpy as np
import pytest

from tests import pointwise_mlp_layers_oracle as O
from tests.host_emul.host_build import P, aligned, load, nans, run_sanitizer_program, sanitizer_program, transposed_table

cf = ctypes.c_float


@pytest.fixture(scope="module")
def host():
    return load("pointwise_mlp_layers", ["pointwise_mlp_layers"])


def fold(case):
    """W[0] (D_in, H) -> w_pos, W_c = W_fi - W_df, W_n = W_df + W_fj"""
    mode, W, C = case["mode"], case["W"][0], case["f"].shape[1]
    o, wp, wc = 0, None, None
    if mode.startswith("dp"):
        wp, o = W[:3], 3
    if "fi_df" in mode:
        wi, wd = W[o:o + C], W[o + C:o + 2 * C]
        o += 2 * C
        wc = wi - wd
        wn = wd + W[o:o + C] if mode.endswith("fj") else wd
    else:
        wn = W[o:o + C]
    return wp, wc, wn


def split(packed, widths):
    out, o = [], 0
    for w in widths:
        out.append(packed[o:o + w])
        o += w
    return out


def run(L, case, reduction, activation, bn="batch", backward=True, momentum=0.98, eps=1e-3):
    """forward (+ backward) through the C entry points -> dict(out, grad_f, grad_W, grad_gamma, grad_beta, moving_mean, moving_var (lists over the layers),
    raw = the kernels' own outputs)"""
    q, s, idx, f, go = case["q"], case["s"], case["idx"], case["f"], aligned(case["go"])
    n0, C = f.shape
    n, K = idx.shape
    W = case["W"]
    H, C_out, layers = W[0].shape[1], W[-1].shape[1], len(W) - 1
    widths = [w.shape[1] for w in W]
    WT = sum(widths)
    wp, wc, wn = fold(case)
    w_pos = None if wp is None else aligned(wp)
    cen = None if wc is None else aligned(f @ wc)
    nbr = aligned(f @ wn)
    hw = aligned(np.concatenate([w.reshape(-1) for w in W[1:]]))
    bn_mode = {"batch": 1, "moving": 2, None: 0}[bn]
    cat = lambda key: aligned(np.concatenate(case[key])) if bn_mode else None
    gamma, beta, mm, mv = cat("gamma"), cat("beta"), cat("moving_mean"), cat("moving_var")
    save_mean, save_invstd = (nans(WT), nans(WT)) if bn_mode else (None, None)
    pad = np.array([int(idx.max())], np.int32)
    act, red = O.ACTIVATIONS[activation], O.REDUCTIONS[reduction]
    nbytes = L.cbl_pointwise_mlp_layers_workspace_bytes(n, n0, K, H, C_out, layers)
    assert nbytes > 0
    ws = aligned(np.full(nbytes, 0xff, np.uint8))
    out = nans(n, C_out)
    rc = L.cbl_pointwise_mlp_layers_forward(n, n0, K, H, C_out, P(q), P(s), P(idx), P(cen), P(nbr), P(w_pos), cf(case["radius"]), layers, P(hw), bn_mode,
                                            P(gamma), P(beta), cf(eps), cf(momentum), P(mm), P(mv), act, red, P(pad), P(save_mean), P(save_invstd), P(out),
                                            P(ws), ctypes.c_size_t(nbytes), None)
    assert rc == 0
    res = dict(out=out, raw=[out] + ([save_mean, save_invstd, mm, mv] if bn_mode else []))
    if bn_mode:
        res.update(moving_mean=split(mm, widths), moving_var=split(mv, widths))
    if not backward:
        return res
    inv_start, inv_src = transposed_table(idx, n0)
    g_cen = None if cen is None else nans(n, H)
    g_nbr = nans(n0, H)
    g_wp = None if w_pos is None else nans(3, H)
    g_hw = nans(hw.size)
    g_gamma, g_beta = (nans(WT), nans(WT)) if bn_mode else (None, None)
    ws[...] = 0xff                                                   # (nothing of the forward's workspace is needed)
    rc = L.cbl_pointwise_mlp_layers_backward_csr(n, n0, K, H, C_out, P(q), P(s), P(idx), P(cen), P(nbr), P(w_pos), cf(case["radius"]), layers, P(hw), bn_mode,
                                                 P(gamma), P(beta), P(save_mean), P(save_invstd), act, red, P(pad), P(out), P(go), None, P(inv_start),
                                                 P(inv_src), P(g_cen), P(g_nbr), P(g_wp), P(g_hw), P(g_gamma), P(g_beta), P(ws), ctypes.c_size_t(nbytes), None)
    assert rc == 0
    res["raw"] += [g for g in (g_cen, g_nbr, g_wp, g_hw, g_gamma, g_beta) if g is not None]
    # the chain the mirror leaves to autograd: per-query centre rows scattered through idx[:, 0], then the two dense products
    f64 = f.astype(np.float64)
    gn = g_nbr.astype(np.float64)
    grad_f = gn @ wn.T.astype(np.float64)
    blocks = []
    if wp is not None:
        blocks.append(g_wp.astype(np.float64))
    if wc is not None:
        gc = np.zeros((n0 + 1, H))
        np.add.at(gc, idx[:, 0], g_cen.astype(np.float64))
        gc = gc[:n0]
        grad_f = grad_f + gc @ wc.T.astype(np.float64)
        g_wc, g_wn = f64.T @ gc, f64.T @ gn
        blocks += [g_wc, g_wn - g_wc] + ([g_wn] if case["mode"].endswith("fj") else [])
    else:
        blocks.append(f64.T @ gn)
    grad_W, o = [np.concatenate(blocks, 0)], 0
    for w in W[1:]:
        grad_W.append(g_hw[o:o + w.size].reshape(w.shape))
        o += w.size
    res.update(grad_f=grad_f, grad_W=grad_W)
    if bn_mode:
        res.update(grad_gamma=split(g_gamma, widths), grad_beta=split(g_beta, widths))
    return res


@pytest.mark.parametrize("bn", O.BNS)
@pytest.mark.parametrize("mode", O.MODES)
@pytest.mark.parametrize("fc_num", O.FC_NUMS)
def test_every_depth_mode_reduction_and_bn_mode(host, fc_num, mode, bn):
    """base shape, relu, one query without any neighbour and up to 30 % trailing shadow entries: out, every gradient and (batch statistics) every layer's
    moving statistics under sum, mean and max"""
    case = O.base_case(fc_num, mode)
    for reduction in ("sum", "mean", "max"):
        ref = O.reference(case, reduction, "relu", bn)
        O.assert_flip_free(ref, reduction, "relu")
        res = run(host, case, reduction, "relu", bn)
        O.check(res, ref, bn, "%s %s" % (reduction, bn))
        if bn == "moving":                                           # evaluation leaves the moving statistics alone
            for got, was in zip(res["moving_mean"] + res["moving_var"], case["moving_mean"] + case["moving_var"]):
                np.testing.assert_array_equal(got, was)


@pytest.mark.parametrize("activation,mode", [("leaky_relu", "dp_fj"), ("none", "dp_fi_df")])
def test_leaky_relu_and_identity(host, activation, mode):
    for fc_num in O.FC_NUMS:
        case = O.base_case(fc_num, mode)
        for reduction in ("sum", "max"):
            ref = O.reference(case, reduction, activation)
            O.assert_flip_free(ref, reduction, activation)
            O.check(run(host, case, reduction, activation), ref, "batch", activation + " " + reduction)


@pytest.mark.parametrize("n0,n,K,C,C_out", O.SHAPES)
def test_shapes(host, n0, n, K, C, C_out):
    """gradients for sum / mean with the identity (no flip possible at any size), forward with relu under max; 'dp_fi_df_fj', batch statistics, beta != 0"""
    for fc_num in O.FC_NUMS:
        case = O.make_case(n0, n, K, C, C_out, 3, "dp_fi_df_fj", fc_num, all_shadow_row=n > 1)
        for reduction in ("sum", "mean"):
            O.check(run(host, case, reduction, "none"), O.reference(case, reduction, "none"), "batch", reduction)
        res = run(host, case, "max", "relu", backward=False)
        O.check(res, O.reference(case, "max", "relu", backward=False), "batch", "relu max")


@pytest.mark.parametrize("fc_num,mode", sorted(O.SEEDS_MEAN_8))
def test_features_of_mean_8(host, fc_num, mode):
    """|mean y_0| is many standard deviations of y_0: variance by E[y^2] - E[y]^2 in fp32 would leave no digits (fp64 sums)"""
    case = O.make_case(*O.BASE, O.SEEDS_MEAN_8[(fc_num, mode)], mode, fc_num, offset=8.0)
    ref = O.reference(case, "max", "relu")
    O.assert_flip_free(ref, "max", "relu")
    O.check(run(host, case, "max", "relu"), ref, "batch")
    O.check(run(host, case, "mean", "none"), O.reference(case, "mean", "none"), "batch")


@pytest.mark.parametrize("mode", ["dp_fj", "dp_fi_df"])
def test_hub_target(host, mode):
    """support point 0 owns 300 pairs, more than a tile has rows: the target pass continues it over several chunks"""
    n0 = O.HUB[0]
    for fc_num in O.FC_NUMS:
        case = O.random_case(*O.HUB, 1, mode, fc_num, hub=True)
        assert np.bincount(case["idx"].reshape(-1), minlength=n0 + 1)[0] > 256
        for reduction, bn in (("sum", "batch"), ("mean", None)):
            O.check(run(host, case, reduction, "none", bn), O.reference(case, reduction, "none", bn), bn, reduction)


@pytest.mark.parametrize("fc_num", O.FC_NUMS)
def test_mean_without_any_padding_counts_the_largest_index_as_padding(host, fc_num):
    """:609-613 — nn counts idx < max(idx): without a shadow entry anywhere the largest REAL index is left out of nn, but not of the mask"""
    case = O.make_case(*O.BASE, 2, "dp_fj", fc_num, padding=False)
    assert case["idx"].max() < O.BASE[0]
    O.check(run(host, case, "mean", "none"), O.reference(case, "mean", "none"), "batch")


@pytest.mark.parametrize("bn", O.BNS)
def test_a_query_whose_neighbours_are_all_shadow(host, bn):
    """its pairs are in every layer's statistics, its output is 0 under every reduction ('max' of zeros, 0 / 1e-5); every output finite"""
    case = O.base_case(3, "dp_fi_df")
    assert (case["idx"][0] == O.BASE[0]).all()
    for reduction in ("max", "sum", "mean"):
        res = run(host, case, reduction, "leaky_relu", bn)
        assert (res["out"][0] == 0).all()
        assert all(np.isfinite(g).all() for g in res["raw"])
        O.close(res["out"], O.reference(case, reduction, "leaky_relu", bn, backward=False)["out"])


def test_more_trips_than_every_grid_cap(host):
    """O.CAPS: K = 4 at H = 16 and C_out = 4 — every query-side pass takes more than 512 trips (the caps), the target side at least 519.
    Forward + gradients, identity activation, batch statistics"""
    for fc_num in O.FC_NUMS:
        case = O.random_case(*O.CAPS, 4, "dp_fj", fc_num, pad_frac=0.25)
        O.check(run(host, case, "sum", "none"), O.reference(case, "sum", "none"), "batch")


def test_two_calls_give_identical_bits(host):
    case = O.make_case(96, 48, 10, 36, 72, 0, "dp_fi_df_fj", 3)
    for reduction, activation, bn in (("max", "relu", "batch"), ("mean", "leaky_relu", "moving"), ("sum", "none", None)):
        a = run(host, case, reduction, activation, bn)["raw"]
        b = run(host, case, reduction, activation, bn)["raw"]
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


def test_unsupported_and_bad_arguments(host):
    """outside the limits: CBL_ERR_UNSUPPORTED (-3) and a workspace size of 0; a NULL input: CBL_ERR_BAD_ARG (-1) before any launch; empty: a no-op"""
    n0, n, K = 96, 8, 10
    case = O.make_case(n0, n, K, 32, 32, 0, "dp_fj", 2)
    q, s = case["q"], case["s"]
    idx = np.full((n, 129), n0, np.int32)
    nbr, hw, out, pad = np.zeros((n0, 148), np.float32), np.zeros(148 * 148 + 148 * 1028, np.float32), nans(n, 1028), np.array([n0], np.int32)
    size = host.cbl_pointwise_mlp_layers_workspace_bytes

    def fwd(n=n, K=K, H=16, C_out=32, layers=1, hw=hw, out=out, q=q, radius=0.15, red=0, act=0):
        return host.cbl_pointwise_mlp_layers_forward(n, n0, K, H, C_out, P(q), P(s), P(idx), None, P(nbr), None, cf(radius), layers, P(hw), 0, None, None,
                                                     cf(1e-3), cf(0.98), None, None, act, red, P(pad), None, None, P(out), None, ctypes.c_size_t(0), None)
    for kw in (dict(layers=0), dict(layers=3), dict(H=9), dict(H=15), dict(H=145), dict(K=129), dict(K=49, H=72), dict(C_out=18), dict(C_out=1028)):
        a = dict(K=K, H=16, C_out=32, layers=1)
        a.update(kw)
        assert fwd(**kw) == -3, kw
        assert size(n, n0, a["K"], a["H"], a["C_out"], a["layers"]) == 0, kw
    assert size(n, n0, 48, 144, 288, 2) > 0 and size(n, n0, 128, 64, 1024, 2) > 0 and size(n, n0, K, 16, 4, 1) > 0
    assert fwd(hw=None) == -1 and fwd(out=None) == -1 and fwd(q=None) == -1
    assert fwd(radius=0.0) == -1 and fwd(red=3) == -1 and fwd(act=3) == -1 and fwd(K=0) == -1
    assert fwd(n=0) == 0                                             # empty = no-op
    assert not np.isfinite(out).any()                                # nothing was launched
    ws = aligned(np.zeros(size(n, n0, K, 16, 32, 1), np.uint8))
    g_hw = nans(16 * 32)

    def bwd(layers=1, go=out, H=16, nbytes=ws.nbytes, g_nbr=None):
        return host.cbl_pointwise_mlp_layers_backward_csr(n, n0, K, H, 32, P(q), P(s), P(idx), None, P(nbr), None, cf(0.15), layers, P(hw), 0, None, None, None,
                                                          None, 0, 0, P(pad), P(out), P(go), None, None, None, None, P(g_nbr), None, P(g_hw), None, None,
                                                          P(ws), ctypes.c_size_t(nbytes), None)
    assert bwd(layers=3) == -3 and bwd(H=8) == -3
    assert bwd(go=None) == -1 and bwd(nbytes=16) == -2
    assert bwd(g_nbr=nbr) == -1                                      # grad_neighbor without the transposed table
    assert not np.isfinite(g_hw).any()


def test_the_mirror_refuses_what_the_kernels_do_not_cover():
    """NotImplementedError naming fc_num for depths, widths and neighbour counts outside the kernels and for a fc_num that disagrees with the layers passed;
    ValueError for shapes and for batch-norm variables present on one layer and absent on another — all before any kernel is touched"""
    import torch
    from contrastboundary_amd import local_aggregation as LA
    n0, n = 96, 8
    q, s, f = torch.zeros(n, 3), torch.zeros(n0, 3), torch.zeros(n0, 32)

    def call(H=16, K=10, C_out=32, hidden=1, bn=True, fc_num=None, hidden_bn=None, C=32, last=None):
        idx = torch.zeros((n, K), dtype=torch.int32)
        v = lambda w, on: (torch.ones(w), torch.zeros(w), torch.zeros(w), torch.ones(w)) if on else (None,) * 4
        layers = [(torch.zeros(H, H),) + v(H, bn if hidden_bn is None else hidden_bn) for _ in range(hidden - 1)]
        layers.append((torch.zeros(last or (H, C_out)),) + v(C_out, bn if hidden_bn is None else hidden_bn))
        return LA.pointwise_mlp(q, s, idx, torch.zeros(n0, C), 0.15, torch.zeros(3 + C, H), *v(H, bn), fc_hidden=layers, fc_num=fc_num)
    for kw in (dict(hidden=3), dict(H=9), dict(H=145), dict(K=49, H=72), dict(K=129), dict(fc_num=3), dict(fc_num=1)):
        with pytest.raises(NotImplementedError, match="fc_num"):
            call(**kw)
    for kw in (dict(hidden_bn=False), dict(bn=False, hidden_bn=True), dict(last=(17, 32))):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(NotImplementedError, match="fc_num"):
        LA.pointwise_mlp(None, None, None, None, 0.15, None, fc_num=2)
    with pytest.raises(NotImplementedError, match="fc_num"):
        LA.pointwise_mlp(q, s, torch.zeros((n, 10), dtype=torch.int32), f, 0.15, torch.zeros(35, 16), fc_num=2)
    for kw in (dict(fc_num=4), dict(fc_num=2, in_fdim=12), dict(fc_num=3, in_fdim=300)):
        with pytest.raises(NotImplementedError, match="fc_num"):
            LA.PointWiseMLP(kw.pop("in_fdim", 32), 16, **kw)


def test_the_kernels_under_address_sanitizer():
    """the stand-alone program: the same translation unit with -fsanitize=address,undefined, forward + backward over the shape edges, heap buffers of exactly
    their logical size"""
    r = run_sanitizer_program(sanitizer_program("pointwise_mlp_layers", ["pointwise_mlp_layers"]))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "cases ok" in r.stdout
