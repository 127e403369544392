"""CPU: the PointWiseMLP kernels (contrastboundary_amd/csrc/pointwise_mlp.hip; tensorflow/models/local_aggregation_operators.py:503-617, fc_num 1) compiled for
the HOST and run with wave semantics (tests/host_emul/wave), through their C entry points, against the float64 restatement of the graph code in its direct
form (tests/pointwise_mlp_oracle.py) within the 1e-4 contract.  The fold of the FC weights into per-point terms and the chain back to the features and the
weights are done here as the Python mirror does them (contrastboundary_amd/local_aggregation.pointwise_mlp), in numpy.
Gradient cases with an activation or 'max' assert, from the oracle, that no ReLU / arg-max flip between fp32 and float64 can occur (seeds chosen so)."""
import ctypes

import numpy as np
import pytest

from tests import pointwise_mlp_oracle as O
from tests.host_emul.host_build import P, aligned, load, nans, transposed_table

BASE = (96, 48, 10, 12, 16)                                          # n0, n, K, C, C_out
SEED = {"dp_fj": 1, "fi_df": 0, "dp_fi_df": 0, "dp_fi_df_fj": 2}      # flip-free at BASE for features of mean 0 and of mean 8 (asserted per case)
cf = ctypes.c_float


@pytest.fixture(scope="module")
def host():
    return load("pointwise_mlp", ["pointwise_mlp"])


def fold(case):
    """W (D_in, C_out) -> w_pos, W_c = W_fi - W_df, W_n = W_df + W_fj and the row ranges they came from"""
    mode, W, C = case["mode"], case["W"], case["f"].shape[1]
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


def run(L, case, reduction, activation, bn="batch", backward=True, momentum=0.98, eps=1e-3):
    """forward (+ backward) through the C entry points -> dict(out, grad_f, grad_W, grad_gamma, grad_beta, moving_mean, moving_var, raw=the kernels' own outputs)"""
    q, s, idx, f, go = case["q"], case["s"], case["idx"], case["f"], aligned(case["go"])
    n0, C = f.shape
    n, K = idx.shape
    C_out = case["W"].shape[1]
    wp, wc, wn = fold(case)
    w_pos = None if wp is None else aligned(wp)
    cen = None if wc is None else aligned(f @ wc)
    nbr = aligned(f @ wn)
    bn_mode = {"batch": 1, "moving": 2, None: 0}[bn]
    gamma, beta = (aligned(case["gamma"]), aligned(case["beta"])) if bn_mode else (None, None)
    mm, mv = (aligned(case["moving_mean"]), aligned(case["moving_var"])) if bn_mode else (None, None)
    save_mean, save_invstd = (nans(C_out), nans(C_out)) if bn_mode else (None, None)
    pad = np.array([int(idx.max())], np.int32)
    act, red = O.ACTIVATIONS[activation], O.REDUCTIONS[reduction]
    nbytes = L.cbl_pointwise_mlp_workspace_bytes(n, n0, K, C_out)
    assert nbytes > 0
    ws = aligned(np.zeros(nbytes, np.uint8))
    out = nans(n, C_out)
    rc = L.cbl_pointwise_mlp_forward(n, n0, K, C_out, P(q), P(s), P(idx), P(cen), P(nbr), P(w_pos), cf(case["radius"]), bn_mode, P(gamma), P(beta), cf(eps),
                                     cf(momentum), P(mm), P(mv), act, red, P(pad), P(save_mean), P(save_invstd), P(out), P(ws), ctypes.c_size_t(nbytes), None)
    assert rc == 0
    res = dict(out=out, moving_mean=mm, moving_var=mv, raw=[out, save_mean, save_invstd])
    if not backward:
        return res
    inv_start, inv_src = transposed_table(idx, n0)
    g_cen = None if cen is None else nans(n, C_out)
    g_nbr = nans(n0, C_out)
    g_wp = None if w_pos is None else nans(3, C_out)
    g_gamma, g_beta = (nans(C_out), nans(C_out)) if bn_mode else (None, None)
    ws[...] = 0xff                                                   # (nothing of the forward's workspace is needed)
    rc = L.cbl_pointwise_mlp_backward_csr(n, n0, K, C_out, P(q), P(s), P(idx), P(cen), P(nbr), P(w_pos), cf(case["radius"]), bn_mode, P(gamma), P(beta),
                                          P(save_mean), P(save_invstd), act, red, P(pad), P(out), P(go), None, P(inv_start), P(inv_src),
                                          P(g_cen), P(g_nbr), P(g_wp), P(g_gamma), P(g_beta), P(ws), ctypes.c_size_t(nbytes), None)
    assert rc == 0
    res["raw"] += [g_cen, g_nbr, g_wp, g_gamma, g_beta]
    # the chain the mirror leaves to autograd: per-query centre rows scattered through idx[:, 0], then the two dense products
    f64 = f.astype(np.float64)
    gn = g_nbr.astype(np.float64)
    grad_f = gn @ wn.T.astype(np.float64)
    blocks = []
    if wp is not None:
        blocks.append(g_wp.astype(np.float64))
    if wc is not None:
        gc = np.zeros((n0 + 1, C_out))
        np.add.at(gc, idx[:, 0], g_cen.astype(np.float64))
        gc = gc[:n0]
        grad_f = grad_f + gc @ wc.T.astype(np.float64)
        g_wc, g_wn = f64.T @ gc, f64.T @ gn
        blocks += [g_wc, g_wn - g_wc] + ([g_wn] if case["mode"].endswith("fj") else [])
    else:
        blocks.append(f64.T @ gn)
    res.update(grad_f=grad_f, grad_W=np.concatenate(blocks, 0), grad_gamma=g_gamma, grad_beta=g_beta)
    return res


def check(res, ref, bn="batch", what=""):
    O.close(res["out"], ref["out"], what + " out")
    if "grad_f" in res:
        O.close(res["grad_f"], ref["grad_f"], what + " grad features")
        O.close(res["grad_W"], ref["grad_W"], what + " grad weights")
        if bn:
            O.close(res["grad_gamma"], ref["grad_gamma"], what + " grad gamma")
            O.close(res["grad_beta"], ref["grad_beta"], what + " grad beta")


@pytest.mark.parametrize("activation", ["relu", "leaky_relu", "none"])
@pytest.mark.parametrize("reduction", ["max", "sum", "mean"])
@pytest.mark.parametrize("mode", O.MODES)
def test_training_every_mode_reduction_activation(host, mode, reduction, activation):
    """batch statistics over all n*K pairs (shadow pairs included, one query without any neighbour), output, every gradient, the moving statistics"""
    case = O.make_case(*BASE, SEED[mode], mode)
    ref = O.reference(case, reduction, activation)
    O.assert_flip_free(ref, reduction, activation)
    res = run(host, case, reduction, activation)
    check(res, ref)
    O.close(res["moving_mean"], ref["moving_mean"], "moving mean")
    O.close(res["moving_var"], ref["moving_var"], "moving variance")


@pytest.mark.parametrize("reduction,activation", [("max", "relu"), ("mean", "leaky_relu"), ("sum", "none")])
@pytest.mark.parametrize("mode", O.MODES)
def test_features_of_mean_8(host, mode, reduction, activation):
    """|mean y| is many standard deviations of y: the statistics pass must not lose the variance (fp64 sums)"""
    case = O.make_case(*BASE, SEED[mode], mode, offset=8.0)
    ref = O.reference(case, reduction, activation)
    O.assert_flip_free(ref, reduction, activation)
    check(run(host, case, reduction, activation), ref)


@pytest.mark.parametrize("n0,n,K,C,C_out", [(96, 48, 5, 12, 16), (96, 48, 33, 12, 16), (96, 48, 10, 12, 4), (96, 48, 10, 12, 72), (96, 1, 10, 12, 16)])
def test_shapes(host, n0, n, K, C, C_out):
    """K below and above a lane's unroll, one float4 column and 18 of them (several workgroups per pass), a single query; the smooth configurations carry
    the gradient check on every shape (no flip possible), 'relu' + 'max' the forward"""
    case = O.make_case(n0, n, K, C, C_out, 3, "dp_fi_df_fj", all_shadow_row=n > 1)
    for reduction in ("sum", "mean"):
        check(run(host, case, reduction, "none"), O.reference(case, reduction, "none"), what=reduction)
    res = run(host, case, "max", "relu", backward=False)
    O.close(res["out"], O.reference(case, "max", "relu")["out"], "max out")


def test_a_query_whose_neighbours_are_all_shadow(host):
    """its pairs are in the statistics (dp = -q / radius, the centre row is the shadow row), its output is 0 under every reduction ('max' of zeros, 0 / 1e-5)"""
    case = O.make_case(*BASE, 1, "dp_fi_df")
    assert (case["idx"][0] == BASE[0]).all()
    for reduction in ("max", "sum", "mean"):
        res = run(host, case, reduction, "leaky_relu", backward=False)
        assert (res["out"][0] == 0).all()
        O.close(res["out"], O.reference(case, reduction, "leaky_relu")["out"])


@pytest.mark.parametrize("mode", ["dp_fj", "dp_fi_df_fj"])
def test_mean_without_any_padding_counts_the_largest_index_as_padding(host, mode):
    """:609-613 — nn counts idx < max(idx): without a shadow entry anywhere the largest REAL index is left out of nn, but not of the mask"""
    case = O.make_case(*BASE, 2, mode, padding=False)
    assert case["idx"].max() < BASE[0]
    ref = O.reference(case, "mean", "none")
    check(run(host, case, "mean", "none"), ref)
    has = (case["idx"] == case["idx"].max()).any(1)
    assert has.any() and not has.all()


@pytest.mark.parametrize("bn", ["moving", None])
@pytest.mark.parametrize("reduction,activation", [("max", "relu"), ("mean", "leaky_relu"), ("sum", "none")])
def test_evaluation_mode_and_no_batch_norm(host, bn, reduction, activation):
    """moving statistics (constants under the gradient) and bn=False: one forward pass, no coupling of the pairs in the backward"""
    mode = "dp_fi_df"
    case = O.make_case(*BASE, SEED[mode], mode)
    ref = O.reference(case, reduction, activation, bn=bn)
    O.assert_flip_free(ref, reduction, activation)
    res = run(host, case, reduction, activation, bn=bn)
    check(res, ref, bn=bn)
    if bn == "moving":                                               # evaluation leaves the moving statistics alone
        np.testing.assert_array_equal(res["moving_mean"], case["moving_mean"])
        np.testing.assert_array_equal(res["moving_var"], case["moving_var"])


def test_moving_statistics_follow_the_tf_convention(host):
    """moving = moving * momentum + batch * (1 - momentum) with the BIASED batch variance (torch's running_var takes the unbiased one)"""
    case = O.make_case(*BASE, 1, "dp_fj", offset=8.0)
    for momentum in (0.98, 0.5):
        ref = O.reference(case, "sum", "relu", momentum=momentum)
        res = run(host, case, "sum", "relu", backward=False, momentum=momentum)
        O.close(res["moving_mean"], ref["moving_mean"])
        O.close(res["moving_var"], ref["moving_var"])
    N = BASE[1] * BASE[2]
    batch_var = (ref["moving_var"] - case["moving_var"] * 0.5) / 0.5
    unbiased = case["moving_var"] * 0.5 + batch_var * N / (N - 1) * 0.5
    assert np.abs(res["moving_var"] - unbiased).max() > 1e-4 * np.abs(unbiased).max()        # the two conventions are told apart at this size


def test_two_calls_give_identical_bits(host):
    case = O.make_case(96, 48, 10, 12, 72, 0, "dp_fi_df_fj")
    for reduction, activation in (("max", "relu"), ("mean", "leaky_relu")):
        a = run(host, case, reduction, activation)["raw"]
        b = run(host, case, reduction, activation)["raw"]
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


def test_unsupported_and_bad_arguments(host):
    """outside the limits: CBL_ERR_UNSUPPORTED (-3); bad arguments: CBL_ERR_BAD_ARG (-1), before any launch; fc_num > 1: NotImplementedError naming the option"""
    case = O.make_case(*BASE, 0, "dp_fj")
    q, s, idx = case["q"], case["s"], case["idx"]
    n0, n, K, C, C_out = BASE
    nbr, out, pad = nans(n0, C_out), nans(n, C_out), np.array([n0], np.int32)

    def fwd(n=n, K=K, C_out=C_out, nbr=nbr, radius=0.15, red=0, act=0):
        return host.cbl_pointwise_mlp_forward(n, n0, K, C_out, P(q), P(s), P(idx), None, P(nbr), None, cf(radius), 0, None, None, cf(1e-3), cf(0.98), None, None,
                                              act, red, P(pad), None, None, P(out), None, ctypes.c_size_t(0), None)
    assert fwd(C_out=18) == -3                                       # C_out % 4 != 0
    assert fwd(K=129) == -3                                          # K > 128
    assert fwd(C_out=1028) == -3
    assert host.cbl_pointwise_mlp_workspace_bytes(n, n0, 129, C_out) == 0
    assert fwd(nbr=None) == -1
    assert fwd(radius=0.0) == -1
    assert fwd(red=3) == -1 and fwd(act=3) == -1 and fwd(K=0) == -1
    assert fwd(n=0) == 0                                             # empty = no-op
    assert not np.isfinite(out).any()
    ws = aligned(np.zeros(host.cbl_pointwise_mlp_workspace_bytes(n, n0, K, C_out), np.uint8))

    def bwd(K=K, C_out=C_out, go=out, nbytes=ws.nbytes):
        return host.cbl_pointwise_mlp_backward_csr(n, n0, K, C_out, P(q), P(s), P(idx), None, P(nbr), None, cf(0.15), 0, None, None, None, None, 0, 0, P(pad),
                                                   P(out), P(go), None, None, None, None, P(nbr), None, None, None, P(ws), ctypes.c_size_t(nbytes), None)
    assert bwd(K=129) == -3 and bwd(C_out=18) == -3
    assert bwd(go=None) == -1
    assert bwd() == -1                                               # grad_neighbor without the transposed table
    from contrastboundary_amd import local_aggregation as LA
    with pytest.raises(NotImplementedError, match="fc_num"):
        LA.PointWiseMLP(12, 16, fc_num=2)
    with pytest.raises(NotImplementedError, match="fc_num"):
        LA.pointwise_mlp(None, None, None, None, 0.15, None, fc_num=2)
