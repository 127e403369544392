"""CPU: the general AdaptiveWeight kernels (contrastboundary_amd/csrc/adaptive_weight_general.hip; tensorflow/models/local_aggregation_operators.py:316-500,
fc_num 1: every local_input_feature, shared_channels, weight_softmax, sum / mean / max) compiled for the HOST and run with wave semantics
(tests/host_emul/wave), through their C entry points, against the float64 restatement of the graph code in its direct form
(tests/adaptive_weight_general_oracle.py; restatement only, TensorFlow absent) within the 1e-4 contract.  The fold of the FC weights into per-point terms and
the chain back to the features and the weights are done here as the Python mirror does them (contrastboundary_amd/local_aggregation.adaptive_weight), in
numpy.  Every 'max' gradient case asserts, from the oracle, that no arg-max flip between fp32 and float64 can occur (seeds chosen so)."""
import ctypes

import numpy as np
import pytest

from tests import adaptive_weight_general_oracle as O
from tests.host_emul.host_build import P, aligned, load, nans, transposed_table

cf = ctypes.c_float


@pytest.fixture(scope="module")
def host():
    return load("adaptive_weight_general", ["adaptive_weight_general"])


def run(L, case, softmax, reduction, backward=True):
    """forward (+ backward) through the C entry points -> dict(out, grad_f, grad_W, grad_b, raw=the kernels' own outputs)"""
    q, s, idx, f, go = case["q"], case["s"], case["idx"], aligned(case["f"]), aligned(case["go"])
    n0, C = f.shape
    n, K = idx.shape
    M = C // case["S"]
    wp, wc, wn = O.fold(case)
    w_pos = None if wp is None else np.ascontiguousarray(wp)
    cen = None if wc is None else np.ascontiguousarray(f @ wc)
    nbr = None if wn is None else np.ascontiguousarray(f @ wn)
    bias = case["b"]
    pad = np.array([int(idx.max())], np.int32)
    sm, red = O.SOFTMAX[softmax], O.REDUCTIONS[reduction]
    nbytes = L.cbl_adaptive_weight_general_workspace_bytes(n, n0, K, C, M)
    assert nbytes > 0
    ws = aligned(np.full(nbytes, 0xff, np.uint8))
    out = nans(n, C)
    rc = L.cbl_adaptive_weight_general_forward(n, n0, K, C, M, P(q), P(s), P(idx), P(f), P(cen), P(nbr), P(w_pos), P(bias), cf(case["radius"]), sm, red,
                                               P(pad), P(out), P(ws), ctypes.c_size_t(nbytes), None)
    assert rc == 0
    res = dict(out=out, raw=[out])
    if not backward:
        return res
    inv_start, inv_src = transposed_table(idx, n0)
    g_val, g_cen, g_nbr, g_wp, g_b = nans(n0, C), nans(n, M), nans(n0, M), nans(3, M), nans(M)
    rc = L.cbl_adaptive_weight_general_backward_csr(n, n0, K, C, M, P(q), P(s), P(idx), P(f), P(cen), P(nbr), P(w_pos), P(bias), cf(case["radius"]), sm, red,
                                                    P(pad), P(out), P(go), None, P(inv_start), P(inv_src), P(g_val), P(g_cen), P(g_nbr), P(g_wp), P(g_b),
                                                    P(ws), ctypes.c_size_t(nbytes), None)
    assert rc == 0
    res["raw"] += [g_val, g_cen, g_nbr, g_wp, g_b]
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
    res.update(grad_f=grad_f, grad_W=O.unfold(case, g_wp.astype(np.float64), g_wc, g_wn), grad_b=g_b)
    return res


@pytest.mark.parametrize("reduction", ["sum", "mean", "max"])
@pytest.mark.parametrize("softmax", O.SOFTMAXES)
@pytest.mark.parametrize("S", O.SHARED)
@pytest.mark.parametrize("mode", O.MODES)
def test_every_mode_group_softmax_reduction(host, mode, S, softmax, reduction):
    """base shape with one query without any neighbour and up to 30 % trailing shadow entries: out and the gradients of features, fc_weight, fc_bias"""
    case = O.base_case(mode, S, softmax)
    ref = O.reference(case, softmax, reduction)
    O.assert_flip_free(ref, reduction)
    O.check(run(host, case, softmax, reduction), ref, case, softmax)


@pytest.mark.parametrize("n0,n,K,C,S", O.SHAPES)
def test_shapes(host, n0, n, K, C, S):
    """forward for the three reductions, gradients for sum / mean (nothing can flip), 'dp_fi_df', masked softmax"""
    case = O.make_case(n0, n, K, C, 3, "dp_fi_df", S, all_shadow_row=n > 1)
    for reduction in ("sum", "mean"):
        O.check(run(host, case, "dense", reduction), O.reference(case, "dense", reduction), case, "dense", reduction)
    res = run(host, case, "dense", "max", backward=False)
    O.check(res, O.reference(case, "dense", "max", backward=False), case, "dense", "max")


@pytest.mark.parametrize("softmax", O.SOFTMAXES)
def test_a_query_whose_neighbours_are_all_shadow(host, softmax):
    """0 under sum / mean, -65535 under max; every gradient finite (a masked softmax over no pair gives zero weights, not 0 / 0)"""
    case = O.base_case("dp_fi_df", 4, softmax)
    assert (case["idx"][0] == O.BASE[0]).all()
    for reduction in ("sum", "mean", "max"):
        res = run(host, case, softmax, reduction)
        assert (res["out"][0] == (-65535.0 if reduction == "max" else 0.0)).all()
        for g in res["raw"]:
            assert np.isfinite(g).all()


@pytest.mark.parametrize("softmax", [None, "dense"])
def test_mean_without_any_padding_counts_the_largest_index_as_padding(host, softmax):
    """:466-470 — nn counts idx < max(idx): without a shadow entry anywhere the largest REAL index is left out of nn, but not of the sum"""
    case = O.make_case(*O.BASE, 2, "dp_fj", 2, padding=False)
    assert case["idx"].max() < O.BASE[0]
    O.check(run(host, case, softmax, "mean"), O.reference(case, softmax, "mean"), case, softmax)
    has = (case["idx"] == case["idx"].max()).any(1)
    assert has.any() and not has.all()


def test_masked_softmax_spellings_and_unmask(host):
    """'dense', 'sparse', 'mask': one masked softmax, identical bits; 'unmask' (shadow pairs take part with a real logit) is another function"""
    case = O.base_case("dp_fj", 2, "dense")
    ref_m, ref_u = O.reference(case, "dense", "sum"), O.reference(case, "unmask", "sum")
    assert np.abs(ref_m["out"] - ref_u["out"]).max() > 1e-3 * np.abs(ref_m["out"]).max()           # the oracle tells the two apart
    a = run(host, case, "dense", "sum")
    for other in ("sparse", "mask"):
        np.testing.assert_array_equal(O.reference(case, other, "sum")["out"], ref_m["out"])
        for x, y in zip(a["raw"], run(host, case, other, "sum")["raw"]):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
    u = run(host, case, "unmask", "sum")
    assert np.abs(u["out"] - a["out"]).max() > 1e-3 * np.abs(a["out"]).max()
    O.check(u, ref_u, case, "unmask")


@pytest.mark.parametrize("softmax", ["dense", "unmask"])
def test_logits_that_overflow_a_plain_exponential(host, softmax):
    """weights x 20 and bias + 80: exp(y) is past fp32 (y reaches beyond 88), the running maximum keeps every exponent at or below 0"""
    case = O.make_case(*O.BASE, 0, "dp_fj", 2, scale=20.0, shift=80.0)
    y = np.concatenate([(case["s"][np.minimum(case["idx"], O.BASE[0] - 1)] - case["q"][:, None]) / case["radius"],
                        case["f"][np.minimum(case["idx"], O.BASE[0] - 1)]], -1) @ case["W"] + case["b"]
    assert y.max() > 89.0
    for reduction in ("sum", "mean", "max"):
        res = run(host, case, softmax, reduction, backward=reduction != "max")
        assert all(np.isfinite(g).all() for g in res["raw"])
        O.check(res, O.reference(case, softmax, reduction), case, softmax, reduction)


@pytest.mark.parametrize("S", [1, 8])
def test_medium(host, S):
    """every pass spans many workgroups: forward for the three reductions, gradients for sum / mean, 'max' twice with identical bits in every output"""
    case = O.make_case(*O.MEDIUM, 5, "dp_fj", S, pad_frac=0.4)
    for reduction in ("sum", "mean"):
        O.check(run(host, case, "dense", reduction), O.reference(case, "dense", reduction), case, "dense", reduction)
    a = run(host, case, "dense", "max")
    O.check(dict(out=a["out"]), O.reference(case, "dense", "max", backward=False), case, "dense", "max")
    b = run(host, case, "dense", "max")
    for x, y in zip(a["raw"], b["raw"]):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.isfinite(a["grad_f"]).all() and np.abs(a["grad_f"]).max() > 0


def test_two_calls_give_identical_bits(host):
    case = O.make_case(96, 48, 10, 72, 0, "dp_fi_df", 24)
    for softmax, reduction in ((None, "max"), ("dense", "mean"), ("unmask", "sum")):
        a = run(host, case, softmax, reduction)["raw"]
        b = run(host, case, softmax, reduction)["raw"]
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("reduction", ["sum", "mean"])
def test_the_shipped_configuration_through_the_general_entries(host, reduction):
    """'dp', shared_channels 1, no softmax: what cbl_adaptive_weight_* compute (oracle/local_aggregation_oracle.adaptive_weight and its gradients)"""
    from oracle import local_aggregation_oracle as LO
    case = O.base_case("dp", 1, None)
    args = (case["q"], case["s"], case["idx"], case["f"], case["radius"], case["W"], case["b"])
    res = run(host, case, None, reduction)
    O.close(res["out"], LO.adaptive_weight(*args, reduction=reduction))
    gf, gw, gb = LO.adaptive_weight_grads(*args, case["go"], reduction=reduction)
    O.close(res["grad_f"], gf); O.close(res["grad_W"], gw); O.close(res["grad_b"], gb)


def test_unsupported_and_bad_arguments(host):
    """outside the limits: CBL_ERR_UNSUPPORTED (-3); bad arguments: CBL_ERR_BAD_ARG (-1), before any launch; the mirror's refusals name the option"""
    case = O.base_case("dp", 1, None)
    q, s, idx, f = case["q"], case["s"], case["idx"], aligned(case["f"])
    n0, n, K, C = O.BASE
    bias, out, pad = np.zeros(1152, np.float32), nans(n, C), np.array([n0], np.int32)
    size = host.cbl_adaptive_weight_general_workspace_bytes

    def fwd(n=n, K=K, C=C, M=C, bias=bias, out=out, radius=0.15, sm=0, red=0, f=f):
        return host.cbl_adaptive_weight_general_forward(n, n0, K, C, M, P(q), P(s), P(idx), P(f), None, None, None, P(bias), cf(radius), sm, red, P(pad), P(out),
                                                        None, ctypes.c_size_t(0), None)
    assert fwd(C=18, M=18) == -3                                     # C % 4 != 0
    assert fwd(K=129) == -3                                          # K > 128
    assert fwd(C=1156, M=1156) == -3                                 # C > 1152
    assert fwd(M=5) == -3                                            # C % M != 0
    assert fwd(M=4) == -3 and fwd(C=24, M=4) == -3                   # shared_channels 3 and 6: neither 1, 2, 4 nor a multiple of 4
    assert fwd(f=f.reshape(-1)[1:-3]) == -3                          # rows not 16-byte aligned
    assert size(n, n0, 129, C, C) == 0 and size(n, n0, K, C, 4) == 0 and size(n, n0, K, C, C) > 0
    assert fwd(radius=0.0) == -1 and fwd(bias=None) == -1 and fwd(out=None) == -1
    assert fwd(sm=3) == -1 and fwd(red=3) == -1 and fwd(K=0) == -1 and fwd(M=0) == -1
    assert fwd(n=0) == 0                                             # empty = no-op
    assert not np.isfinite(out).any()
    ws = aligned(np.zeros(size(n, n0, K, C, C), np.uint8))
    g_val, g_nbr, g_b = nans(n0, C), nans(n0, C), nans(C)
    inv_start, inv_src = transposed_table(idx, n0)

    def bwd(K=K, M=C, go=out, radius=0.15, table=True, g_val=g_val, g_nbr=g_nbr, nbytes=ws.nbytes):
        return host.cbl_adaptive_weight_general_backward_csr(n, n0, K, C, M, P(q), P(s), P(idx), P(f), None, None, None, P(bias), cf(radius), 0, 0, P(pad), P(out),
                                                             P(go), None, P(inv_start) if table else None, P(inv_src) if table else None, P(g_val), None,
                                                             P(g_nbr), None, P(g_b), P(ws), ctypes.c_size_t(nbytes), None)
    assert bwd(K=129) == -3 and bwd(M=4) == -3
    assert bwd(go=None) == -1 and bwd(radius=0.0) == -1
    assert bwd(table=False) == -1 and bwd(table=False, g_nbr=None) == -1 and bwd(table=False, g_val=None) == -1     # the (n0, .) gradients without a table
    assert bwd(nbytes=16) == -2
    assert not np.isfinite(g_b).any()                                # nothing was launched
    out[...] = 0
    assert bwd(table=False, g_val=None, g_nbr=None) == 0 and np.isfinite(g_b).all()     # the per-query gradients need no table
    from contrastboundary_amd import local_aggregation as LA
    for kw, exc, match in ((dict(local_input_feature="rscnn"), NotImplementedError, "rscnn"), (dict(local_input_feature="gac"), NotImplementedError, "gac"),
                           (dict(weight_softmax="softmax"), NotImplementedError, "weight_softmax"),
                           (dict(shared_channels=5), NotImplementedError, "shared_channels"), (dict(shared_channels=3), NotImplementedError, "shared_channels"),
                           (dict(local_input_feature="dp_fj"), ValueError, "fc_weight")):
        with pytest.raises(exc, match=match):
            LA.adaptive_weight(None, None, None, np.zeros((n0, C), np.float32), 0.15, np.zeros((3, C), np.float32), None, "sum", **kw)
