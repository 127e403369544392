"""CPU: the AdaptiveWeight kernels for fc_num 2 and 3 (contrastboundary_amd/csrc/adaptive_weight_mlp.hip; tensorflow/models/local_aggregation_operators.py:316-500
with the layers of :419-430) compiled for the HOST and run with wave semantics (tests/host_emul/wave: the MFMA chain is emulated in its own lane layout),
through their C entry points, against the float64 restatement of the graph code in its direct form (tests/adaptive_weight_mlp_oracle.py) within the 1e-4
contract.  The fold of the first layer into per-point terms and the chain back to the features and the first layer's weights are done here in numpy, as the
Python mirror leaves them to autograd.  The workspace is poisoned with 0xff and every output with NaN before each call.  Gradient cases with an activation or
'max' assert, from the oracle, that no relu or arg-max can flip between fp32 and float64 (seeds chosen so).
A stand-alone AddressSanitizer program (tests/host_emul/adaptive_weight_mlp_asan_main.cpp) runs the same translation unit over the shape edges with heap
buffers of exactly their logical size: an indexing error of a kernel surfaces there, on the CPU."""
import ctypes

import numpy as np
import pytest

from tests import adaptive_weight_general_oracle as G
from tests import adaptive_weight_mlp_oracle as O
from tests.host_emul.host_build import P, aligned, load, nans, run_sanitizer_program, sanitizer_program, transposed_table

cf = ctypes.c_float
ACT = {"relu": 1, "leaky_relu": 2}
# the grid caps and the most targets of a target-side trip (AWM_F_BLOCKS, AWM_BQ_BLOCKS, AWM_BT_BLOCKS of the kernel file, PAIR_TPT_MAX of pair_tile.h)
F_BLOCKS, BQ_BLOCKS, BT_BLOCKS, TPT_MAX = 1024, 1024, 1024, 16


@pytest.fixture(scope="module")
def host():
    return load("adaptive_weight_mlp", ["adaptive_weight_mlp"])


def run(L, case, softmax, reduction, backward=True):
    """forward (+ backward) through the C entry points -> dict(out, grad_f, grad_W, grad_b, grad_hw, grad_hb, raw=the kernels' own outputs)"""
    q, s, idx, f, go = case["q"], case["s"], case["idx"], aligned(case["f"]), aligned(case["go"])
    n0, C = f.shape
    n, K = idx.shape
    M = C // case["S"]
    layers = len(case["hw"])
    wp, wc, wn = G.fold(case)
    w_pos = None if wp is None else np.ascontiguousarray(wp)
    cen = None if wc is None else np.ascontiguousarray(f @ wc)
    nbr = None if wn is None else np.ascontiguousarray(f @ wn)
    bias, hw, hb = case["b"], np.ascontiguousarray(np.stack(case["hw"])), np.ascontiguousarray(np.stack(case["hb"]))
    act = ACT.get(case["activation"], 0)
    pad = np.array([int(idx.max())], np.int32)
    sm, red = O.SOFTMAX[softmax], O.REDUCTIONS[reduction]
    nbytes = L.cbl_adaptive_weight_mlp_workspace_bytes(n, n0, K, C, M, layers)
    assert nbytes > 0
    ws = aligned(np.full(nbytes, 0xff, np.uint8))
    out = nans(n, C)
    rc = L.cbl_adaptive_weight_mlp_forward(n, n0, K, C, M, P(q), P(s), P(idx), P(f), P(cen), P(nbr), P(w_pos), P(bias), layers, P(hw), P(hb), act,
                                           cf(case["radius"]), sm, red, P(pad), P(out), P(ws), ctypes.c_size_t(nbytes), None)
    assert rc == 0
    res = dict(out=out, raw=[out])
    if not backward:
        return res
    inv_start, inv_src = transposed_table(idx, n0)
    g_val, g_cen, g_nbr, g_wp, g_b = nans(n0, C), nans(n, M), nans(n0, M), nans(3, M), nans(M)
    g_hw, g_hb = nans(layers, M, M), nans(layers, M)
    rc = L.cbl_adaptive_weight_mlp_backward_csr(n, n0, K, C, M, P(q), P(s), P(idx), P(f), P(cen), P(nbr), P(w_pos), P(bias), layers, P(hw), P(hb), act,
                                                cf(case["radius"]), sm, red, P(pad), P(out), P(go), None, P(inv_start), P(inv_src), P(g_val),
                                                P(g_cen) if cen is not None else None, P(g_nbr) if nbr is not None else None,
                                                P(g_wp) if w_pos is not None else None, P(g_b), P(g_hw), P(g_hb), P(ws), ctypes.c_size_t(nbytes), None)
    assert rc == 0
    res["raw"] += [g_val, g_b, g_hw, g_hb] + [g for g, have in ((g_cen, cen), (g_nbr, nbr), (g_wp, w_pos)) if have is not None]
    # the chain the mirror leaves to autograd: per-query centre rows scattered through idx[:, 0], then the two dense products
    f64 = f.astype(np.float64)
    grad_f = g_val.astype(np.float64)
    g_wc = g_wn = None
    if wn is not None:
        gn = g_nbr.astype(np.float64)
        grad_f = grad_f + gn @ wn.T.astype(np.float64)
        g_wn = f64.T @ gn
    if wc is not None:
        gc = np.zeros((n0 + 1, M))
        np.add.at(gc, idx[:, 0], g_cen.astype(np.float64))
        gc = gc[:n0]
        grad_f = grad_f + gc @ wc.T.astype(np.float64)
        g_wc = f64.T @ gc
    res.update(grad_f=grad_f, grad_W=G.unfold(case, g_wp.astype(np.float64), g_wc, g_wn), grad_b=g_b, grad_hw=list(g_hw), grad_hb=list(g_hb))
    return res


@pytest.mark.parametrize("fc_num", O.FC_NUMS)
@pytest.mark.parametrize("softmax", O.SOFTMAXES)
@pytest.mark.parametrize("S", O.SHARED)
@pytest.mark.parametrize("mode", O.MODES)
def test_every_mode_group_softmax_reduction_depth(host, mode, S, softmax, fc_num):
    """base shape, relu, one query without any neighbour and up to 30 % trailing shadow entries: out and every gradient under sum, mean and max"""
    case = O.base_case(fc_num, mode, S, softmax)
    for reduction in ("sum", "mean", "max"):
        ref = O.reference(case, softmax, reduction)
        O.assert_flip_free(ref, case, reduction)
        O.check(run(host, case, softmax, reduction), ref, case, softmax, reduction)


@pytest.mark.parametrize("activation,mode", [("leaky_relu", "dp_fj"), ("none", "dp_fi_df")])
def test_leaky_relu_and_identity(host, activation, mode):
    for fc_num in O.FC_NUMS:
        case = O.flip_free_case("dense", ("sum", "max"), mode, 2, fc_num, activation)
        for reduction in ("sum", "max"):
            ref = O.reference(case, "dense", reduction)
            O.assert_flip_free(ref, case, reduction)
            O.check(run(host, case, "dense", reduction), ref, case, "dense", activation + " " + reduction)


@pytest.mark.parametrize("n0,n,K,C,S", O.SHAPES)
def test_shapes(host, n0, n, K, C, S):
    """forward for the three reductions, gradients for sum / mean; 'dp_fi_df', masked softmax, identity activation for the gradients (at these sizes no
    seed keeps every relu away from 0), relu for one forward"""
    for fc_num in O.FC_NUMS:
        case = O.make_case(n0, n, K, C, 3, "dp_fi_df", S, fc_num, "none", all_shadow_row=n > 1)
        for reduction in ("sum", "mean"):
            O.check(run(host, case, "dense", reduction), O.reference(case, "dense", reduction), case, "dense", reduction)
        res = run(host, case, "dense", "max", backward=False)
        O.check(res, O.reference(case, "dense", "max", backward=False), case, "dense", "max")
        case = O.make_case(n0, n, K, C, 3, "dp_fi_df", S, fc_num, "relu", all_shadow_row=n > 1)
        O.check(run(host, case, "dense", "sum", backward=False), O.reference(case, "dense", "sum", backward=False), case, "dense", "relu sum")


@pytest.mark.parametrize("mode", ["dp", "dp_fj"])
def test_hub_targets(host, mode):
    """8 support points, 384 pairs: every target owns more pairs than one row tile, the target pass continues a target over several chunks"""
    n0, n, K, C, S = O.HUB
    for fc_num in O.FC_NUMS:
        case = O.hub_case(1, mode, fc_num)
        assert np.bincount(case["idx"].reshape(-1), minlength=n0 + 1)[:n0].min() > 16
        for softmax, reduction in ((None, "sum"), ("dense", "mean")):
            O.check(run(host, case, softmax, reduction), O.reference(case, softmax, reduction), case, softmax, reduction)


@pytest.mark.parametrize("softmax", O.SOFTMAXES)
def test_a_query_whose_neighbours_are_all_shadow(host, softmax):
    """0 under sum / mean, -65535 under max; every gradient finite"""
    case = O.base_case(3, "dp_fi_df", 2, softmax)
    assert (case["idx"][0] == O.BASE[0]).all()
    for reduction in ("sum", "mean", "max"):
        res = run(host, case, softmax, reduction)
        assert (res["out"][0] == (-65535.0 if reduction == "max" else 0.0)).all()
        for g in res["raw"]:
            assert np.isfinite(g).all()


@pytest.mark.parametrize("softmax", [None, "dense"])
def test_mean_without_any_padding_counts_the_largest_index_as_padding(host, softmax):
    """:466-470 — nn counts idx < max(idx): without a shadow entry anywhere the largest REAL index is left out of nn, but not of the sum"""
    case = O.make_case(*O.BASE, 2, "dp_fj", 2, 2, "none", padding=False)
    assert case["idx"].max() < O.BASE[0]
    O.check(run(host, case, softmax, "mean"), O.reference(case, softmax, "mean"), case, softmax)


@pytest.mark.parametrize("softmax", ["dense", "unmask"])
def test_logits_that_overflow_a_plain_exponential(host, softmax):
    """last layer's weights x 20 and bias + 80: exp(y) is past fp32, the running maximum keeps every exponent at or below 0"""
    case = O.make_case(*O.BASE, 0, "dp_fj", 2, 2, "none", last_scale=20.0, last_shift=80.0)
    for reduction in ("sum", "mean", "max"):
        res = run(host, case, softmax, reduction, backward=reduction != "max")
        assert all(np.isfinite(g).all() for g in res["raw"])
        O.check(res, O.reference(case, softmax, reduction, backward=reduction != "max"), case, softmax, reduction)


def test_more_trips_than_every_grid_cap(host):
    """K = 128 at M = 16: at most two queries per trip (256 rows), so 2100 queries are at least 1050 trips (caps 1024; the query pass of the backward keeps
    that cap while its partials are small, as here); a target-side trip takes at most 16 targets, so 17000 targets are at least 1063 trips (cap 1024).
    Forward + gradients, identity activation"""
    n0, n, K, C = 17000, 2100, 128, 16
    assert n // (256 // K) > max(F_BLOCKS, BQ_BLOCKS) and -(-n0 // TPT_MAX) > BT_BLOCKS
    case = O.make_case(n0, n, K, C, 4, "dp_fj", 1, 2, "none", pad_frac=0.1)
    O.check(run(host, case, "dense", "sum"), O.reference(case, "dense", "sum"), case, "dense")


def test_two_calls_give_identical_bits(host):
    case = O.make_case(96, 48, 10, 72, 0, "dp_fi_df", 4, 3)
    for softmax, reduction in ((None, "max"), ("dense", "mean"), ("unmask", "sum")):
        a = run(host, case, softmax, reduction)["raw"]
        b = run(host, case, softmax, reduction)["raw"]
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


def test_unsupported_and_bad_arguments(host):
    """outside the limits: CBL_ERR_UNSUPPORTED (-3) and a workspace size of 0; a NULL input: CBL_ERR_BAD_ARG (-1) before any launch"""
    n0, n, K = 96, 8, 10
    case = O.make_case(n0, n, K, 144, 0, "dp", 1, 2)
    q, s, f = case["q"], case["s"], aligned(case["f"])
    idx = np.full((n, 129), n0, np.int32)
    bias, hw, hb, out, pad = np.zeros(1152, np.float32), np.zeros(3 * 148 * 148, np.float32), np.zeros(3 * 148, np.float32), nans(n, 1152), np.array([n0], np.int32)
    size = host.cbl_adaptive_weight_mlp_workspace_bytes

    def fwd(K=K, C=32, M=32, layers=1, hw=hw, out=out, q=q):
        return host.cbl_adaptive_weight_mlp_forward(n, n0, K, C, M, P(q), P(s), P(idx), P(f), None, None, None, P(bias), layers, P(hw), P(hb), 1, cf(0.15), 0, 0,
                                                    P(pad), P(out), None, ctypes.c_size_t(0), None)
    for kw in (dict(layers=0), dict(layers=3), dict(C=12, M=12), dict(C=148, M=148), dict(K=129), dict(K=64, C=144, M=144)):
        a = dict(K=K, C=32, M=32, layers=1)
        a.update(kw)
        assert fwd(**kw) == -3, kw
        assert size(n, n0, a["K"], a["C"], a["M"], a["layers"]) == 0, kw
    assert size(n, n0, 48, 144, 144, 2) > 0 and size(n, n0, 128, 64, 64, 2) > 0 and size(n, n0, K, 64, 16, 1) > 0
    assert fwd(hw=None) == -1 and fwd(out=None) == -1 and fwd(q=None) == -1
    assert not np.isfinite(out).any()                                # nothing was launched
    ws = aligned(np.zeros(size(n, n0, K, 32, 32, 1), np.uint8))
    g_b = nans(32)

    def bwd(layers=1, go=out, M=32, nbytes=ws.nbytes):
        return host.cbl_adaptive_weight_mlp_backward_csr(n, n0, K, 32, M, P(q), P(s), P(idx), P(f), None, None, None, P(bias), layers, P(hw), P(hb), 1, cf(0.15),
                                                         0, 0, P(pad), P(out), P(go), None, None, None, None, None, None, None, P(g_b), None, None, P(ws),
                                                         ctypes.c_size_t(nbytes), None)
    assert bwd(layers=3) == -3 and bwd(M=8) == -3
    assert bwd(go=None) == -1 and bwd(nbytes=16) == -2
    assert not np.isfinite(g_b).any()


def test_the_kernels_under_address_sanitizer():
    """the stand-alone program: the same translation unit with -fsanitize=address,undefined, forward + backward over the shape edges, heap buffers of exactly
    their logical size"""
    r = run_sanitizer_program(sanitizer_program("adaptive_weight_mlp", ["adaptive_weight_mlp"]))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "cases ok" in r.stdout
