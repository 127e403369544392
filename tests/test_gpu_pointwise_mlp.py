"""GPU: PointWiseMLP (contrastboundary_amd/local_aggregation.pointwise_mlp over csrc/pointwise_mlp.hip; tensorflow/models/local_aggregation_operators.py:503-617,
fc_num 1) through the Python mirror with autograd, against the float64 restatement of the graph code in its direct form (tests/pointwise_mlp_oracle.py;
parity unpinned by execution — TF absent) within the 1e-4 contract.  The small cases of tests/test_pointwise_mlp_host.py again on the device, and one shape
at which every pass spans many workgroups.  Gradient cases with an activation or 'max' assert the oracle's no-flip precondition (seeds chosen so)."""
import functools

import numpy as np
import pytest
import torch

from tests import pointwise_mlp_oracle as O

pytestmark = pytest.mark.gpu

BASE = (96, 48, 10, 12, 16)                                          # n0, n, K, C, C_out
SEED = {"dp_fj": 1, "fi_df": 0, "dp_fi_df": 0, "dp_fi_df_fj": 2}      # flip-free at BASE for features of mean 0 and of mean 8 (asserted per case)
MEDIUM = (3000, 1500, 26, 72, 72)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def medium_case():
    case = O.make_case(*MEDIUM, 5, "dp_fi_df_fj", pad_frac=0.4)      # 0 .. 10 trailing shadow entries per row: about 20 % padding
    frac = (case["idx"] == MEDIUM[0]).mean()
    assert 0.15 < frac < 0.25
    return case


@functools.lru_cache(maxsize=None)
def medium_reference(reduction, activation):
    return O.reference(medium_case(), reduction, activation)


def run(case, reduction, activation, bn="batch", backward=True, momentum=0.98):
    from contrastboundary_amd import local_aggregation as LA
    f, W = dev(case["f"]).requires_grad_(backward), dev(case["W"]).requires_grad_(backward)
    gamma = beta = mm = mv = None
    if bn:
        gamma, beta = dev(case["gamma"]).requires_grad_(backward), dev(case["beta"]).requires_grad_(backward)
        mm, mv = dev(case["moving_mean"]), dev(case["moving_var"])
    out = LA.pointwise_mlp(dev(case["q"]), dev(case["s"]), dev(case["idx"]), f, case["radius"], W, gamma, beta, mm, mv, local_input_feature=case["mode"],
                           reduction=reduction, activation_fn=activation, is_training=bn != "moving", bn_momentum=momentum)
    res = dict(out=out.detach().cpu().numpy())
    if bn:
        res.update(moving_mean=mm.cpu().numpy(), moving_var=mv.cpu().numpy())
    if backward:
        out.backward(dev(case["go"]))
        res.update(grad_f=f.grad.cpu().numpy(), grad_W=W.grad.cpu().numpy())
        if bn:
            res.update(grad_gamma=gamma.grad.cpu().numpy(), grad_beta=beta.grad.cpu().numpy())
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
def test_training_every_mode_reduction_activation(mode, reduction, activation):
    case = O.make_case(*BASE, SEED[mode], mode)
    ref = O.reference(case, reduction, activation)
    O.assert_flip_free(ref, reduction, activation)
    res = run(case, reduction, activation)
    check(res, ref)
    O.close(res["moving_mean"], ref["moving_mean"], "moving mean")
    O.close(res["moving_var"], ref["moving_var"], "moving variance")


@pytest.mark.parametrize("reduction,activation", [("max", "relu"), ("mean", "leaky_relu"), ("sum", "none")])
@pytest.mark.parametrize("mode", O.MODES)
def test_features_of_mean_8(mode, reduction, activation):
    case = O.make_case(*BASE, SEED[mode], mode, offset=8.0)
    ref = O.reference(case, reduction, activation)
    O.assert_flip_free(ref, reduction, activation)
    check(run(case, reduction, activation), ref)


@pytest.mark.parametrize("n0,n,K,C,C_out", [(96, 48, 5, 12, 16), (96, 48, 33, 12, 16), (96, 48, 10, 12, 4), (96, 48, 10, 12, 72), (96, 1, 10, 12, 16)])
def test_shapes(n0, n, K, C, C_out):
    case = O.make_case(n0, n, K, C, C_out, 3, "dp_fi_df_fj", all_shadow_row=n > 1)
    for reduction in ("sum", "mean"):
        check(run(case, reduction, "none"), O.reference(case, reduction, "none"), what=reduction)
    res = run(case, "max", "relu", backward=False)
    O.close(res["out"], O.reference(case, "max", "relu")["out"], "max out")


def test_mean_without_any_padding_counts_the_largest_index_as_padding():
    case = O.make_case(*BASE, 2, "dp_fi_df_fj", padding=False)
    assert case["idx"].max() < BASE[0]
    check(run(case, "mean", "none"), O.reference(case, "mean", "none"))


@pytest.mark.parametrize("bn", ["moving", None])
@pytest.mark.parametrize("reduction,activation", [("max", "relu"), ("mean", "leaky_relu"), ("sum", "none")])
def test_evaluation_mode_and_no_batch_norm(bn, reduction, activation):
    mode = "dp_fi_df"
    case = O.make_case(*BASE, SEED[mode], mode)
    ref = O.reference(case, reduction, activation, bn=bn)
    O.assert_flip_free(ref, reduction, activation)
    res = run(case, reduction, activation, bn=bn)
    check(res, ref, bn=bn)
    if bn == "moving":
        np.testing.assert_array_equal(res["moving_mean"], case["moving_mean"])
        np.testing.assert_array_equal(res["moving_var"], case["moving_var"])


def test_module_holds_the_variables_and_follows_its_training_flag():
    from contrastboundary_amd import local_aggregation as LA
    mode = "dp_fi_df_fj"
    case = O.make_case(*BASE, SEED[mode], mode)
    m = LA.PointWiseMLP(BASE[3], BASE[4], local_input_feature=mode, fc_num=1, reduction="mean", activation_fn="leaky_relu").cuda()
    assert tuple(m.weights.shape) == case["W"].shape and float(m.weights.detach().abs().max()) > 0
    assert sorted(k for k, _ in m.named_buffers()) == ["moving_mean", "moving_variance"]
    with torch.no_grad():
        m.weights.copy_(dev(case["W"])); m.gamma.copy_(dev(case["gamma"])); m.beta.copy_(dev(case["beta"]))
        m.moving_mean.copy_(dev(case["moving_mean"])); m.moving_variance.copy_(dev(case["moving_var"]))
    args = (dev(case["q"]), dev(case["s"]), dev(case["idx"]), dev(case["f"]), case["radius"])
    ref = O.reference(case, "mean", "leaky_relu")
    out = m(*args)
    O.close(out.detach().cpu().numpy(), ref["out"])
    O.close(m.moving_mean.cpu().numpy(), ref["moving_mean"])
    O.close(m.moving_variance.cpu().numpy(), ref["moving_var"])
    out.backward(dev(case["go"]))
    O.close(m.weights.grad.cpu().numpy(), ref["grad_W"])
    m.eval()
    ev = dict(case, moving_mean=m.moving_mean.cpu().numpy(), moving_var=m.moving_variance.cpu().numpy())
    O.close(m(*args).detach().cpu().numpy(), O.reference(ev, "mean", "leaky_relu", bn="moving")["out"])


def test_options_outside_the_kernels_are_refused():
    from contrastboundary_amd import local_aggregation as LA
    case = O.make_case(*BASE, 0, "dp_fj")
    q, s, idx, f = dev(case["q"]), dev(case["s"]), dev(case["idx"]), dev(case["f"])
    with pytest.raises(NotImplementedError, match="fc_num"):
        LA.pointwise_mlp(q, s, idx, f, 0.15, dev(case["W"]), fc_num=2)
    with pytest.raises(NotImplementedError):
        LA.pointwise_mlp(q, s, idx, f, 0.15, dev(case["W"][:, :6]))                                # C_out % 4 != 0
    with pytest.raises(NotImplementedError):
        LA.pointwise_mlp(q, s, dev(np.zeros((BASE[1], 129), np.int32)), f, 0.15, dev(case["W"]))   # K > 128
    with pytest.raises(NotImplementedError):
        LA.pointwise_mlp(q, s, idx, f, 0.15, dev(case["W"]), local_input_feature="dp")
    with pytest.raises(NotImplementedError):
        LA.pointwise_mlp(q, s, idx, f, 0.15, dev(case["W"]), reduction="avg")


# ---------------------------------------------------------------- a shape at which every pass spans many workgroups
@pytest.mark.parametrize("activation", ["relu", "leaky_relu", "none"])
@pytest.mark.parametrize("reduction", ["max", "sum", "mean"])
def test_medium_forward(reduction, activation):
    res = run(medium_case(), reduction, activation, backward=False)
    ref = medium_reference(reduction, activation)
    O.close(res["out"], ref["out"])
    O.close(res["moving_mean"], ref["moving_mean"])
    O.close(res["moving_var"], ref["moving_var"])


@pytest.mark.parametrize("reduction", ["sum", "mean"])
def test_medium_gradients_of_the_smooth_configurations(reduction):
    """no activation, no maximum: nothing can flip, 1e-4 holds for every gradient (features, weights, gamma, beta)"""
    check(run(medium_case(), reduction, "none"), medium_reference(reduction, "none"))


def test_medium_relu_max_forward_and_a_bit_identical_backward():
    a = run(medium_case(), "max", "relu")
    O.close(a["out"], medium_reference("max", "relu")["out"])
    b = run(medium_case(), "max", "relu")
    for k in ("out", "grad_f", "grad_W", "grad_gamma", "grad_beta", "moving_mean", "moving_var"):
        np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32), err_msg=k)
    assert np.isfinite(a["grad_f"]).all() and np.abs(a["grad_f"]).max() > 0


def test_on_a_side_stream():
    mode = "dp_fi_df"
    case = O.make_case(*BASE, SEED[mode], mode)
    ref = O.reference(case, "mean", "none")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        res = run(case, "mean", "none")
    st.synchronize()
    check(res, ref)
