"""GPU: PointWiseMLP with fc_num 2 and 3 (contrastboundary_amd/local_aggregation.pointwise_mlp(..., fc_hidden=...) over csrc/pointwise_mlp_layers.hip;
tensorflow/models/local_aggregation_operators.py:503-617 with the layers of :589-600) through the Python mirror with autograd, against the float64 restatement
of the graph code in its direct form (tests/pointwise_mlp_layers_oracle.py; parity unpinned by execution — TF absent) within the 1e-4 contract.  The cases of
tests/test_pointwise_mlp_layers_host.py again on the device, and what only the mirror has: a side stream, the module, fc_hidden=() against today's call.
Gradient cases with an activation or 'max' assert the oracle's no-flip precondition (seeds chosen so)."""
import functools

import numpy as np
import pytest
import torch

from tests import pointwise_mlp_layers_oracle as O

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def base_reference(fc_num, mode, reduction, activation, bn):
    return O.reference(O.base_case(fc_num, mode), reduction, activation, bn)


def run(case, reduction, activation, bn="batch", backward=True, momentum=0.98):
    """the mirror on the device -> dict(out, grad_f, grad_W, grad_gamma, grad_beta, moving_mean, moving_var (lists over the layers), raw)"""
    from contrastboundary_amd import local_aggregation as LA
    f = dev(case["f"]).requires_grad_(backward)
    W = [dev(w).requires_grad_(backward) for w in case["W"]]
    none = [None] * len(W)
    gamma, beta, mm, mv = none, none, none, none
    if bn:
        gamma, beta = [dev(g).requires_grad_(backward) for g in case["gamma"]], [dev(b).requires_grad_(backward) for b in case["beta"]]
        mm, mv = [dev(m) for m in case["moving_mean"]], [dev(v) for v in case["moving_var"]]
    hidden = [(W[l], gamma[l], beta[l], mm[l], mv[l]) for l in range(1, len(W))]
    out = LA.pointwise_mlp(dev(case["q"]), dev(case["s"]), dev(case["idx"]), f, case["radius"], W[0], gamma[0], beta[0], mm[0], mv[0],
                           local_input_feature=case["mode"], reduction=reduction, activation_fn=activation, is_training=bn != "moving", bn_momentum=momentum,
                           fc_hidden=hidden)
    res = dict(out=out.detach().cpu().numpy())
    if bn:
        res.update(moving_mean=[m.cpu().numpy() for m in mm], moving_var=[v.cpu().numpy() for v in mv])
    if backward:
        out.backward(dev(case["go"]))
        res.update(grad_f=f.grad.cpu().numpy(), grad_W=[w.grad.cpu().numpy() for w in W])
        if bn:
            res.update(grad_gamma=[g.grad.cpu().numpy() for g in gamma], grad_beta=[b.grad.cpu().numpy() for b in beta])
    res["raw"] = [res["out"]] + ([res["grad_f"]] + res["grad_W"] + (res["grad_gamma"] + res["grad_beta"] if bn else []) if backward else []) + \
        (res["moving_mean"] + res["moving_var"] if bn else [])
    return res


@pytest.mark.parametrize("bn", O.BNS)
@pytest.mark.parametrize("mode", O.MODES)
@pytest.mark.parametrize("fc_num", O.FC_NUMS)
def test_every_depth_mode_reduction_and_bn_mode(fc_num, mode, bn):
    """base shape, relu: out, every gradient and (batch statistics) every layer's moving statistics under sum, mean and max"""
    case = O.base_case(fc_num, mode)
    for reduction in ("sum", "mean", "max"):
        ref = base_reference(fc_num, mode, reduction, "relu", bn)
        O.assert_flip_free(ref, reduction, "relu")
        res = run(case, reduction, "relu", bn)
        O.check(res, ref, bn, "%s %s" % (reduction, bn))
        if bn == "moving":                                           # evaluation leaves the moving statistics alone
            for got, was in zip(res["moving_mean"] + res["moving_var"], case["moving_mean"] + case["moving_var"]):
                np.testing.assert_array_equal(got, was)


@pytest.mark.parametrize("activation,mode", [("leaky_relu", "dp_fj"), ("none", "dp_fi_df")])
def test_leaky_relu_and_identity(activation, mode):
    for fc_num in O.FC_NUMS:
        case = O.base_case(fc_num, mode)
        for reduction in ("sum", "max"):
            ref = base_reference(fc_num, mode, reduction, activation, "batch")
            O.assert_flip_free(ref, reduction, activation)
            O.check(run(case, reduction, activation), ref, "batch", activation + " " + reduction)


@pytest.mark.parametrize("n0,n,K,C,C_out", O.SHAPES)
def test_shapes(n0, n, K, C, C_out):
    """gradients for sum / mean with the identity (no flip possible at any size), forward with relu under max; 'dp_fi_df_fj', batch statistics, beta != 0"""
    for fc_num in O.FC_NUMS:
        case = O.make_case(n0, n, K, C, C_out, 3, "dp_fi_df_fj", fc_num, all_shadow_row=n > 1)
        for reduction in ("sum", "mean"):
            O.check(run(case, reduction, "none"), O.reference(case, reduction, "none"), "batch", reduction)
        res = run(case, "max", "relu", backward=False)
        O.check(res, O.reference(case, "max", "relu", backward=False), "batch", "relu max")


@pytest.mark.parametrize("fc_num,mode", sorted(O.SEEDS_MEAN_8))
def test_features_of_mean_8(fc_num, mode):
    """|mean y_0| is many standard deviations of y_0: variance by E[y^2] - E[y]^2 in fp32 would leave no digits (fp64 sums)"""
    case = O.make_case(*O.BASE, O.SEEDS_MEAN_8[(fc_num, mode)], mode, fc_num, offset=8.0)
    ref = O.reference(case, "max", "relu")
    O.assert_flip_free(ref, "max", "relu")
    O.check(run(case, "max", "relu"), ref, "batch")
    O.check(run(case, "mean", "none"), O.reference(case, "mean", "none"), "batch")


@pytest.mark.parametrize("mode", ["dp_fj", "dp_fi_df"])
def test_hub_target(mode):
    """support point 0 owns 300 pairs, more than a tile has rows: the target pass continues it over several chunks"""
    n0 = O.HUB[0]
    for fc_num in O.FC_NUMS:
        case = O.random_case(*O.HUB, 1, mode, fc_num, hub=True)
        assert np.bincount(case["idx"].reshape(-1), minlength=n0 + 1)[0] > 256
        for reduction, bn in (("sum", "batch"), ("mean", None)):
            O.check(run(case, reduction, "none", bn), O.reference(case, reduction, "none", bn), bn, reduction)


@pytest.mark.parametrize("fc_num", O.FC_NUMS)
def test_mean_without_any_padding_counts_the_largest_index_as_padding(fc_num):
    case = O.make_case(*O.BASE, 2, "dp_fj", fc_num, padding=False)
    assert case["idx"].max() < O.BASE[0]
    O.check(run(case, "mean", "none"), O.reference(case, "mean", "none"), "batch")


@pytest.mark.parametrize("bn", O.BNS)
def test_a_query_whose_neighbours_are_all_shadow(bn):
    """its pairs are in every layer's statistics, its output is 0 under every reduction; every output finite"""
    case = O.base_case(3, "dp_fi_df")
    assert (case["idx"][0] == O.BASE[0]).all()
    for reduction in ("max", "sum", "mean"):
        res = run(case, reduction, "leaky_relu", bn)
        assert (res["out"][0] == 0).all()
        assert all(np.isfinite(g).all() for g in res["raw"])
        O.close(res["out"], base_reference(3, "dp_fi_df", reduction, "leaky_relu", bn)["out"])


def test_more_trips_than_every_grid_cap():
    """O.CAPS: K = 4 at H = 16 and C_out = 4 — every query-side pass takes more than 512 trips (the caps), the target side at least 519.
    Forward + gradients, identity activation, batch statistics"""
    for fc_num in O.FC_NUMS:
        case = O.random_case(*O.CAPS, 4, "dp_fj", fc_num, pad_frac=0.25)
        O.check(run(case, "sum", "none"), O.reference(case, "sum", "none"), "batch")


def test_two_calls_give_identical_bits():
    case = O.make_case(96, 48, 10, 36, 72, 0, "dp_fi_df_fj", 3)
    for reduction, activation, bn in (("max", "relu", "batch"), ("mean", "leaky_relu", "moving"), ("sum", "none", None)):
        a = run(case, reduction, activation, bn)["raw"]
        b = run(case, reduction, activation, bn)["raw"]
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


def test_on_a_side_stream():
    case = O.base_case(3, "dp_fi_df_fj")
    ref = base_reference(3, "dp_fi_df_fj", "max", "relu", "batch")
    O.assert_flip_free(ref, "max", "relu")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        res = run(case, "max", "relu")
    side.synchronize()
    O.check(res, ref, "batch")


def test_no_hidden_layer_is_todays_call():
    """fc_hidden=() goes through the fc_num 1 kernels: the bits of the call without the argument"""
    from contrastboundary_amd import local_aggregation as LA
    from tests import pointwise_mlp_oracle as P
    case = P.make_case(96, 48, 10, 12, 16, 1, "dp_fi_df_fj")
    outs = []
    for kw in (dict(), dict(fc_hidden=()), dict(fc_hidden=(), fc_num=1)):
        f, W = dev(case["f"]).requires_grad_(True), dev(case["W"]).requires_grad_(True)
        gamma, beta = dev(case["gamma"]).requires_grad_(True), dev(case["beta"]).requires_grad_(True)
        mm, mv = dev(case["moving_mean"]), dev(case["moving_var"])
        out = LA.pointwise_mlp(dev(case["q"]), dev(case["s"]), dev(case["idx"]), f, case["radius"], W, gamma, beta, mm, mv, local_input_feature=case["mode"], **kw)
        out.backward(dev(case["go"]))
        outs.append([t.detach().cpu().numpy() for t in (out, f.grad, W.grad, gamma.grad, beta.grad, mm, mv)])
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


def test_the_module():
    """parameter names, shapes, init ranges, tf_scopes(); the state_dict of fc_num 1 as it was; a round trip against the oracle"""
    from contrastboundary_amd import local_aggregation as LA
    one = LA.PointWiseMLP(32, 48, "dp_fj")
    assert list(one.state_dict()) == ["weights", "gamma", "beta", "moving_mean", "moving_variance"]
    assert one.tf_scopes() == {k: "fc_1" for k in one.state_dict()}
    assert list(LA.PointWiseMLP(32, 48, "dp_fj", bn=False).state_dict()) == ["weights"]
    torch.manual_seed(0)
    for fc_num in O.FC_NUMS:
        mode = "dp_fi_df_fj"
        C, C_out = O.BASE[3], O.BASE[4]
        H = O.hidden_width(C)
        m = LA.PointWiseMLP(C, C_out, mode, fc_num=fc_num, reduction="max").cuda()
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        want = {"weights": (O.P.d_in(mode, C), H), "gamma": (H,), "beta": (H,), "moving_mean": (H,), "moving_variance": (H,)}
        scopes = {k: "fc_0" for k in want}
        for l in range(1, fc_num):
            w = C_out if l == fc_num - 1 else H
            want.update({"weights_%d" % l: (H, w), "gamma_%d" % l: (w,), "beta_%d" % l: (w,), "moving_mean_%d" % l: (w,), "moving_variance_%d" % l: (w,)})
            scopes.update({k + "_%d" % l: "fc_%d" % (l if l < fc_num - 1 else fc_num) for k in ("weights", "gamma", "beta", "moving_mean", "moving_variance")})
        assert shapes == want
        assert m.tf_scopes() == scopes
        for name, p in m.named_parameters():
            if name.startswith("weights"):
                bound = (6.0 / (p.shape[0] + p.shape[1])) ** 0.5     # xavier, uniform
                assert float(p.detach().abs().max()) <= bound and float(p.detach().std()) > 0.4 * bound
            else:
                assert (p == (1.0 if name.startswith("gamma") else 0.0)).all()
        # the module's own variables as the oracle's case (identity and 'sum': no flip whatever the draw).  gamma, beta and the moving statistics are moved
        # off their initial values first: with beta = 0 and the identity, the batch mean of every layer behind the first is zero in exact arithmetic
        with torch.no_grad():
            for name, p in list(m.named_parameters()) + list(m.named_buffers()):
                if name.startswith("gamma") or name.startswith("moving_variance"):
                    p.uniform_(0.5, 1.5)
                elif not name.startswith("weights"):
                    p.normal_(0.0, 0.3)
        m.reduction, m.activation_fn = "sum", "none"
        case = O.base_case(fc_num, mode)
        tag = lambda l: "" if l == 0 else "_%d" % l
        case["W"] = [getattr(m, "weights" + tag(l)).detach().cpu().numpy() for l in range(fc_num)]
        for key, name in (("gamma", "gamma"), ("beta", "beta"), ("moving_mean", "moving_mean"), ("moving_var", "moving_variance")):
            case[key] = [getattr(m, name + tag(l)).detach().cpu().numpy().copy() for l in range(fc_num)]
        ref = O.reference(case, "sum", "none")
        f = dev(case["f"]).requires_grad_(True)
        out = m(dev(case["q"]), dev(case["s"]), dev(case["idx"]), f, case["radius"])
        out.backward(dev(case["go"]))
        res = dict(out=out.detach().cpu().numpy(), grad_f=f.grad.cpu().numpy(), grad_W=[getattr(m, "weights" + tag(l)).grad.cpu().numpy() for l in range(fc_num)],
                   grad_gamma=[getattr(m, "gamma" + tag(l)).grad.cpu().numpy() for l in range(fc_num)],
                   grad_beta=[getattr(m, "beta" + tag(l)).grad.cpu().numpy() for l in range(fc_num)],
                   moving_mean=[getattr(m, "moving_mean" + tag(l)).cpu().numpy() for l in range(fc_num)],
                   moving_var=[getattr(m, "moving_variance" + tag(l)).cpu().numpy() for l in range(fc_num)])
        O.check(res, ref, "batch", "module fc_num %d" % fc_num)
        m.eval()                                                     # evaluation: the moving statistics, left alone
        before = [b.clone() for b in m.buffers()]
        with torch.no_grad():
            out = m(dev(case["q"]), dev(case["s"]), dev(case["idx"]), dev(case["f"]), case["radius"])
        for key, name in (("moving_mean", "moving_mean"), ("moving_var", "moving_variance")):
            case[key] = [getattr(m, name + tag(l)).cpu().numpy() for l in range(fc_num)]
        O.close(out.cpu().numpy(), O.reference(case, "sum", "none", "moving", backward=False)["out"], "module in evaluation")
        for a, b in zip(before, m.buffers()):
            assert torch.equal(a, b)


def test_the_mirror_refuses_on_the_device_too():
    from contrastboundary_amd import local_aggregation as LA
    q, s, f = torch.zeros(8, 3).cuda(), torch.zeros(96, 3).cuda(), torch.zeros(96, 144).cuda()
    idx = torch.zeros((8, 49), dtype=torch.int32).cuda()
    v = lambda w: (torch.ones(w).cuda(), torch.zeros(w).cuda(), torch.zeros(w).cuda(), torch.ones(w).cuda())
    with pytest.raises(NotImplementedError, match="fc_num"):          # K = 49 at H = 72
        LA.pointwise_mlp(q, s, idx, f, 0.15, torch.zeros(147, 72).cuda(), *v(72), fc_hidden=[(torch.zeros(72, 32).cuda(),) + v(32)])
    with pytest.raises(NotImplementedError, match="fc_num"):
        LA.pointwise_mlp(q, s, idx[:, :10].contiguous(), f, 0.15, torch.zeros(147, 72).cuda(), *v(72), fc_num=2)
    with pytest.raises(ValueError):
        LA.pointwise_mlp(q, s, idx[:, :10].contiguous(), f, 0.15, torch.zeros(147, 72).cuda(), *v(72), fc_hidden=[(torch.zeros(72, 32).cuda(), None, None, None, None)])
