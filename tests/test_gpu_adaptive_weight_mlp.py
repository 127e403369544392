"""GPU: AdaptiveWeight with fc_num 2 and 3 (contrastboundary_amd/local_aggregation.adaptive_weight(..., fc_hidden=...) over csrc/adaptive_weight_mlp.hip;
tensorflow/models/local_aggregation_operators.py:316-500 with the layers of :419-430) through the Python mirror with autograd, against the float64 restatement
of the graph code in its direct form (tests/adaptive_weight_mlp_oracle.py) within the 1e-4 contract.  The cases of tests/test_adaptive_weight_mlp_host.py again on
the device.  Gradient cases with an activation or 'max' assert the oracle's no-flip preconditions (seeds chosen so); at the medium shape no seed can meet
them for 2.8 M pre-activations, so its gradient cases run with the identity activation and its relu cases check the forward."""
import functools

import numpy as np
import pytest
import torch

from tests import adaptive_weight_general_oracle as G
from tests import adaptive_weight_mlp_oracle as O

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(case, softmax, reduction, backward=True):
    from contrastboundary_amd import local_aggregation as LA
    g = lambda a: dev(a).requires_grad_(backward)
    f, W, b = g(case["f"]), g(case["W"]), g(case["b"])
    hidden = [(g(w), g(v)) for w, v in zip(case["hw"], case["hb"])]
    out = LA.adaptive_weight(dev(case["q"]), dev(case["s"]), dev(case["idx"]), f, case["radius"], W, b, reduction, local_input_feature=case["mode"],
                             shared_channels=case["S"], weight_softmax=softmax, fc_hidden=hidden, activation_fn=case["activation"])
    res = dict(out=out.detach().cpu().numpy())
    if backward:
        out.backward(dev(case["go"]))
        res.update(grad_f=f.grad.cpu().numpy(), grad_W=W.grad.cpu().numpy(), grad_b=b.grad.cpu().numpy(), grad_hw=[w.grad.cpu().numpy() for w, _ in hidden],
                   grad_hb=[v.grad.cpu().numpy() for _, v in hidden])
    return res


def arrays(res):
    return [res[k] for k in ("out", "grad_f", "grad_W", "grad_b") if k in res] + res.get("grad_hw", []) + res.get("grad_hb", [])


@functools.lru_cache(maxsize=None)
def medium_case(S, fc_num, activation):
    return O.make_case(*O.MEDIUM, 5, "dp_fj", S, fc_num, activation, pad_frac=0.4)


@functools.lru_cache(maxsize=None)
def medium_reference(S, fc_num, activation, reduction, backward):
    return O.reference(medium_case(S, fc_num, activation), "dense", reduction, backward=backward)


@pytest.mark.parametrize("fc_num", O.FC_NUMS)
@pytest.mark.parametrize("softmax", O.SOFTMAXES)
@pytest.mark.parametrize("S", O.SHARED)
@pytest.mark.parametrize("mode", O.MODES)
def test_every_mode_group_softmax_reduction_depth(mode, S, softmax, fc_num):
    case = O.base_case(fc_num, mode, S, softmax)
    for reduction in ("sum", "mean", "max"):
        ref = O.reference(case, softmax, reduction)
        O.assert_flip_free(ref, case, reduction)
        O.check(run(case, softmax, reduction), ref, case, softmax, reduction)


@pytest.mark.parametrize("activation,mode", [("leaky_relu", "dp_fj"), ("none", "dp_fi_df")])
def test_leaky_relu_and_identity(activation, mode):
    for fc_num in O.FC_NUMS:
        case = O.flip_free_case("dense", ("sum", "max"), mode, 2, fc_num, activation)
        for reduction in ("sum", "max"):
            ref = O.reference(case, "dense", reduction)
            O.assert_flip_free(ref, case, reduction)
            O.check(run(case, "dense", reduction), ref, case, "dense", activation + " " + reduction)


@pytest.mark.parametrize("n0,n,K,C,S", O.SHAPES)
def test_shapes(n0, n, K, C, S):
    for fc_num in O.FC_NUMS:
        case = O.make_case(n0, n, K, C, 3, "dp_fi_df", S, fc_num, "none", all_shadow_row=n > 1)
        for reduction in ("sum", "mean"):
            O.check(run(case, "dense", reduction), O.reference(case, "dense", reduction), case, "dense", reduction)
        O.check(run(case, "dense", "max", backward=False), O.reference(case, "dense", "max", backward=False), case, "dense", "max")
        case = O.make_case(n0, n, K, C, 3, "dp_fi_df", S, fc_num, "relu", all_shadow_row=n > 1)
        O.check(run(case, "dense", "sum", backward=False), O.reference(case, "dense", "sum", backward=False), case, "dense", "relu sum")


@pytest.mark.parametrize("mode", ["dp", "dp_fj"])
def test_hub_targets(mode):
    for fc_num in O.FC_NUMS:
        case = O.hub_case(1, mode, fc_num)
        for softmax, reduction in ((None, "sum"), ("dense", "mean")):
            O.check(run(case, softmax, reduction), O.reference(case, softmax, reduction), case, softmax, reduction)


@pytest.mark.parametrize("softmax", O.SOFTMAXES)
def test_a_query_whose_neighbours_are_all_shadow(softmax):
    case = O.base_case(3, "dp_fi_df", 2, softmax)
    assert (case["idx"][0] == O.BASE[0]).all()
    for reduction in ("sum", "mean", "max"):
        res = run(case, softmax, reduction)
        assert (res["out"][0] == (-65535.0 if reduction == "max" else 0.0)).all()
        assert all(np.isfinite(a).all() for a in arrays(res))


@pytest.mark.parametrize("softmax", [None, "dense"])
def test_mean_without_any_padding_counts_the_largest_index_as_padding(softmax):
    case = O.make_case(*O.BASE, 2, "dp_fj", 2, 2, "none", padding=False)
    assert case["idx"].max() < O.BASE[0]
    O.check(run(case, softmax, "mean"), O.reference(case, softmax, "mean"), case, softmax)


@pytest.mark.parametrize("softmax", ["dense", "unmask"])
def test_logits_that_overflow_a_plain_exponential(softmax):
    case = O.make_case(*O.BASE, 0, "dp_fj", 2, 2, "none", last_scale=20.0, last_shift=80.0)
    for reduction in ("sum", "mean", "max"):
        res = run(case, softmax, reduction, backward=reduction != "max")
        assert all(np.isfinite(a).all() for a in arrays(res))
        O.check(res, O.reference(case, softmax, reduction, backward=reduction != "max"), case, softmax, reduction)


@pytest.mark.parametrize("fc_num", O.FC_NUMS)
@pytest.mark.parametrize("S", [1, 4])
def test_medium_forward_with_relu(S, fc_num):
    for reduction in ("sum", "mean", "max"):
        res = run(medium_case(S, fc_num, "relu"), "dense", reduction, backward=False)
        O.check(res, medium_reference(S, fc_num, "relu", reduction, False), medium_case(S, fc_num, "relu"), "dense", reduction)


@pytest.mark.parametrize("fc_num", O.FC_NUMS)
@pytest.mark.parametrize("S", [1, 4])
def test_medium_gradients_with_the_identity(S, fc_num):
    for reduction in ("sum", "mean"):
        O.check(run(medium_case(S, fc_num, "none"), "dense", reduction), medium_reference(S, fc_num, "none", reduction, True), medium_case(S, fc_num, "none"),
                "dense", reduction)


@pytest.mark.parametrize("reduction", ["max", "sum"])
def test_medium_twice_with_identical_bits(reduction):
    case = medium_case(4, 3, "relu")
    a, b = run(case, "dense", reduction), run(case, "dense", reduction)
    for x, y in zip(arrays(a), arrays(b)):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.isfinite(a["grad_f"]).all() and np.abs(a["grad_f"]).max() > 0


def test_on_a_side_stream():
    case = O.base_case(3, "dp_fi_df", 2, "dense")
    ref = O.reference(case, "dense", "mean")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        res = run(case, "dense", "mean")
    st.synchronize()
    O.check(res, ref, case, "dense")


def test_module_holds_the_variables():
    from contrastboundary_amd import local_aggregation as LA
    case = O.base_case(3, "dp_fi_df", 2, "dense")
    C, M = O.BASE[3], O.BASE[3] // 2
    m = LA.AdaptiveWeight(C, local_input_feature="dp_fi_df", shared_channels=2, fc_num=3, weight_softmax="dense", reduction="sum").cuda()
    assert sorted(k for k, _ in m.named_parameters()) == ["biases", "biases_1", "biases_2", "weights", "weights_1", "weights_2"]
    assert tuple(m.weights.shape) == case["W"].shape
    for l in (1, 2):
        w, b = getattr(m, "weights_%d" % l), getattr(m, "biases_%d" % l)
        assert tuple(w.shape) == (M, M) and tuple(b.shape) == (M,)
        assert float(w.detach().abs().max()) > 0 and float(w.detach().abs().max()) <= 2 * (1.3 / M) ** 0.5 + 1e-6 and float(b.detach().abs().max()) == 0
    assert m.tf_scopes() == {"weights": "fc_0", "biases": "fc_0", "weights_1": "fc_1", "biases_1": "fc_1", "weights_2": "fc_3", "biases_2": "fc_3"}
    assert LA.AdaptiveWeight(C, fc_num=2).tf_scopes() == {"weights": "fc_0", "biases": "fc_0", "weights_1": "fc_2", "biases_1": "fc_2"}
    assert sorted(k for k, _ in LA.AdaptiveWeight(C).named_parameters()) == ["biases", "weights"]
    with torch.no_grad():
        m.weights.copy_(dev(case["W"])); m.biases.copy_(dev(case["b"]))
        for l in (1, 2):
            getattr(m, "weights_%d" % l).copy_(dev(case["hw"][l - 1])); getattr(m, "biases_%d" % l).copy_(dev(case["hb"][l - 1]))
    ref = O.reference(case, "dense", "sum")
    O.assert_flip_free(ref, case, "sum")
    out = m(dev(case["q"]), dev(case["s"]), dev(case["idx"]), dev(case["f"]), case["radius"])
    O.check(dict(out=out.detach().cpu().numpy()), ref, case, "dense")
    out.backward(dev(case["go"]))
    assert all(p.grad is not None for p in m.parameters())
    O.close(m.weights.grad.cpu().numpy(), ref["grad_W"]); O.close(m.biases.grad.cpu().numpy(), ref["grad_b"])
    O.close(m.weights_1.grad.cpu().numpy(), ref["grad_hw"][0]); O.close(m.biases_1.grad.cpu().numpy(), ref["grad_hb"][0])
    O.close(m.weights_2.grad.cpu().numpy(), ref["grad_hw"][1])
    assert float(m.biases_2.grad.abs().max()) == 0


def test_without_hidden_layers_the_call_is_fc_num_1s():
    """fc_hidden=() and an activation_fn: the bits of the call without either, on the general kernels and on the shipped configuration's"""
    from contrastboundary_amd import local_aggregation as LA
    for mode, S, softmax, reduction in (("dp_fi_df", 4, "dense", "max"), ("dp", 1, None, "mean")):
        case = G.base_case(mode, S, softmax)
        args = (dev(case["q"]), dev(case["s"]), dev(case["idx"]), dev(case["f"]), case["radius"], dev(case["W"]), dev(case["b"]), reduction)
        kw = dict(local_input_feature=mode, shared_channels=S, weight_softmax=softmax)
        a = LA.adaptive_weight(*args, **kw)
        b = LA.adaptive_weight(*args, fc_hidden=(), activation_fn="leaky_relu", **kw)
        np.testing.assert_array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))


def test_options_outside_the_kernels_are_refused():
    from contrastboundary_amd import local_aggregation as LA
    case = O.base_case(2, "dp", 1, None)
    q, s, idx, f, W, b = (dev(case[k]) for k in ("q", "s", "idx", "f", "W", "b"))
    hidden = [(dev(case["hw"][0]), dev(case["hb"][0]))]
    with pytest.raises(NotImplementedError, match="fc_num"):
        LA.AdaptiveWeight(32, fc_num=4)
    with pytest.raises(NotImplementedError, match="fc_num"):
        LA.adaptive_weight(q, s, idx, f, 0.15, W, b, "sum", fc_hidden=hidden * 3)
    with pytest.raises(NotImplementedError, match="fc_num"):
        LA.AdaptiveWeight(12, fc_num=2)
    f12, W12, b12 = dev(np.zeros((O.BASE[0], 12), np.float32)), dev(np.zeros((3, 12), np.float32)), dev(np.zeros(12, np.float32))
    with pytest.raises(NotImplementedError, match="fc_num"):
        LA.adaptive_weight(q, s, idx, f12, 0.15, W12, b12, "sum", fc_hidden=[(dev(np.zeros((12, 12), np.float32)), b12)])
    with pytest.raises(NotImplementedError, match="rscnn"):
        LA.adaptive_weight(q, s, idx, f, 0.15, W, b, "sum", local_input_feature="rscnn", fc_hidden=hidden)
    with pytest.raises(NotImplementedError, match="rscnn"):
        LA.AdaptiveWeight(32, local_input_feature="rscnn", fc_num=2)
    with pytest.raises(ValueError, match="fc_hidden"):
        LA.adaptive_weight(q, s, idx, f, 0.15, W, b, "sum", fc_hidden=[(dev(np.zeros((16, 16), np.float32)), dev(np.zeros(16, np.float32)))])
