"""GPU: AdaptiveWeight over its whole option space (contrastboundary_amd/local_aggregation.adaptive_weight over csrc/adaptive_weight_general.hip;
tensorflow/models/local_aggregation_operators.py:316-500, fc_num 1) through the Python mirror with autograd, against the float64 restatement of the graph code
in its direct form (tests/adaptive_weight_general_oracle.py; restatement only, TensorFlow absent) within the 1e-4 contract.  The cases of
tests/test_adaptive_weight_general_host.py again on the device.  Every 'max' gradient case asserts the oracle's no-flip precondition (seeds chosen so)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import adaptive_weight_general_oracle as O

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def medium_case(S):
    case = O.make_case(*O.MEDIUM, 5, "dp_fj", S, pad_frac=0.4)        # 0 .. 10 trailing shadow entries per row: about 20 % padding
    assert 0.15 < (case["idx"] == O.MEDIUM[0]).mean() < 0.25
    return case


@functools.lru_cache(maxsize=None)
def medium_reference(S, reduction):
    return O.reference(medium_case(S), "dense", reduction, backward=reduction != "max")


def run(case, softmax, reduction, backward=True):
    from contrastboundary_amd import local_aggregation as LA
    f, W, b = dev(case["f"]).requires_grad_(backward), dev(case["W"]).requires_grad_(backward), dev(case["b"]).requires_grad_(backward)
    out = LA.adaptive_weight(dev(case["q"]), dev(case["s"]), dev(case["idx"]), f, case["radius"], W, b, reduction, local_input_feature=case["mode"],
                             shared_channels=case["S"], weight_softmax=softmax)
    res = dict(out=out.detach().cpu().numpy())
    if backward:
        out.backward(dev(case["go"]))
        res.update(grad_f=f.grad.cpu().numpy(), grad_W=W.grad.cpu().numpy(), grad_b=b.grad.cpu().numpy())
    return res


@pytest.mark.parametrize("reduction", ["sum", "mean", "max"])
@pytest.mark.parametrize("softmax", O.SOFTMAXES)
@pytest.mark.parametrize("S", O.SHARED)
@pytest.mark.parametrize("mode", O.MODES)
def test_every_mode_group_softmax_reduction(mode, S, softmax, reduction):
    case = O.base_case(mode, S, softmax)
    ref = O.reference(case, softmax, reduction)
    O.assert_flip_free(ref, reduction)
    O.check(run(case, softmax, reduction), ref, case, softmax)


@pytest.mark.parametrize("n0,n,K,C,S", O.SHAPES)
def test_shapes(n0, n, K, C, S):
    case = O.make_case(n0, n, K, C, 3, "dp_fi_df", S, all_shadow_row=n > 1)
    for reduction in ("sum", "mean"):
        O.check(run(case, "dense", reduction), O.reference(case, "dense", reduction), case, "dense", reduction)
    O.check(run(case, "dense", "max", backward=False), O.reference(case, "dense", "max", backward=False), case, "dense", "max")


@pytest.mark.parametrize("softmax", O.SOFTMAXES)
def test_a_query_whose_neighbours_are_all_shadow(softmax):
    case = O.base_case("dp_fi_df", 4, softmax)
    assert (case["idx"][0] == O.BASE[0]).all()
    for reduction in ("sum", "mean", "max"):
        res = run(case, softmax, reduction)
        assert (res["out"][0] == (-65535.0 if reduction == "max" else 0.0)).all()
        for k in ("grad_f", "grad_W", "grad_b"):
            assert np.isfinite(res[k]).all()


@pytest.mark.parametrize("softmax", [None, "dense"])
def test_mean_without_any_padding_counts_the_largest_index_as_padding(softmax):
    case = O.make_case(*O.BASE, 2, "dp_fj", 2, padding=False)
    assert case["idx"].max() < O.BASE[0]
    O.check(run(case, softmax, "mean"), O.reference(case, softmax, "mean"), case, softmax)


def test_masked_softmax_spellings_and_unmask():
    case = O.base_case("dp_fj", 2, "dense")
    ref_m, ref_u = O.reference(case, "dense", "sum"), O.reference(case, "unmask", "sum")
    assert np.abs(ref_m["out"] - ref_u["out"]).max() > 1e-3 * np.abs(ref_m["out"]).max()           # the oracle tells the two apart
    a = run(case, "dense", "sum")
    for other in ("sparse", "mask"):
        o = run(case, other, "sum")
        for k in ("out", "grad_f", "grad_W", "grad_b"):
            np.testing.assert_array_equal(a[k].view(np.uint32), o[k].view(np.uint32), err_msg=other + " " + k)
    u = run(case, "unmask", "sum")
    assert np.abs(u["out"] - a["out"]).max() > 1e-3 * np.abs(a["out"]).max()
    O.check(u, ref_u, case, "unmask")


@pytest.mark.parametrize("softmax", ["dense", "unmask"])
def test_logits_that_overflow_a_plain_exponential(softmax):
    case = O.make_case(*O.BASE, 0, "dp_fj", 2, scale=20.0, shift=80.0)
    for reduction in ("sum", "mean", "max"):
        res = run(case, softmax, reduction, backward=reduction != "max")
        assert all(np.isfinite(v).all() for v in res.values())
        O.check(res, O.reference(case, softmax, reduction), case, softmax, reduction)


@pytest.mark.parametrize("reduction", ["sum", "mean", "max"])
@pytest.mark.parametrize("S", [1, 8])
def test_medium_forward(S, reduction):
    res = run(medium_case(S), "dense", reduction, backward=False)
    O.check(res, medium_reference(S, reduction), medium_case(S), "dense")


@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("S", [1, 8])
def test_medium_gradients(S, reduction):
    O.check(run(medium_case(S), "dense", reduction), medium_reference(S, reduction), medium_case(S), "dense")


@pytest.mark.parametrize("S", [1, 8])
def test_medium_max_twice_with_identical_bits(S):
    a, b = run(medium_case(S), "dense", "max"), run(medium_case(S), "dense", "max")
    for k in ("out", "grad_f", "grad_W", "grad_b"):
        np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32), err_msg=k)
    assert np.isfinite(a["grad_f"]).all() and np.abs(a["grad_f"]).max() > 0


@pytest.mark.parametrize("reduction", ["sum", "mean"])
def test_the_shipped_configuration_through_the_general_entries(reduction):
    """'dp', shared_channels 1, no softmax through cbl_adaptive_weight_general_* : the oracle of the shipped operator, and the present cbl_adaptive_weight_forward"""
    from contrastboundary_amd import _lib, local_aggregation as LA
    from oracle import local_aggregation_oracle as LO
    case = O.base_case("dp", 1, None)
    args = (case["q"], case["s"], case["idx"], case["f"], case["radius"], case["W"], case["b"])
    q, s, idx = dev(case["q"]), dev(case["s"]), dev(case["idx"])
    f, W, b = dev(case["f"]).requires_grad_(), dev(case["W"]).requires_grad_(), dev(case["b"]).requires_grad_()
    out = LA._AdaptiveWeightGeneral.apply(q, s, idx, f, None, None, W, b, case["radius"], 0, O.REDUCTIONS[reduction])
    out.backward(dev(case["go"]))
    ref = LO.adaptive_weight(*args, reduction=reduction)
    O.close(out.detach().cpu().numpy(), ref)
    gf, gw, gb = LO.adaptive_weight_grads(*args, case["go"], reduction=reduction)
    O.close(f.grad.cpu().numpy(), gf); O.close(W.grad.cpu().numpy(), gw); O.close(b.grad.cpu().numpy(), gb)
    n0, n, K, C = O.BASE
    L = _lib.lib()
    pad = torch.empty(1, dtype=torch.int32, device="cuda")
    _lib.check(L.cbl_index_max(ctypes.c_longlong(n * K), _lib.ptr(idx), _lib.ptr(pad), _lib.stream_of(idx)), "cbl_index_max")
    present = torch.empty((n, C), dtype=torch.float32, device="cuda")
    _lib.check(L.cbl_adaptive_weight_forward(n, n0, K, C, _lib.ptr(q), _lib.ptr(s), _lib.ptr(idx), _lib.ptr(f), ctypes.c_float(case["radius"]), _lib.ptr(W),
                                             _lib.ptr(b), _lib.ptr(pad), int(reduction == "mean"), _lib.ptr(present), _lib.stream_of(idx)),
               "cbl_adaptive_weight_forward")
    O.close(out.detach().cpu().numpy(), present.cpu().numpy().astype(np.float64))
    # and the mirror still sends this configuration to the present kernels: their bits
    np.testing.assert_array_equal(LA.adaptive_weight(q, s, idx, f.detach(), case["radius"], W.detach(), b.detach(), reduction).cpu().numpy(), present.cpu().numpy())


def test_on_a_side_stream():
    case = O.base_case("dp_fi_df", 4, "dense")
    ref = O.reference(case, "dense", "mean")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        res = run(case, "dense", "mean")
    st.synchronize()
    O.check(res, ref, case, "dense")


def test_module_holds_the_variables():
    from contrastboundary_amd import local_aggregation as LA
    case = O.base_case("dp_fi_df", 4, "dense")
    m = LA.AdaptiveWeight(O.BASE[3], local_input_feature="dp_fi_df", shared_channels=4, weight_softmax="dense", reduction="max").cuda()
    assert sorted(k for k, _ in m.named_parameters()) == ["biases", "weights"]
    assert tuple(m.weights.shape) == case["W"].shape and float(m.weights.detach().abs().max()) > 0 and float(m.biases.detach().abs().max()) == 0
    with torch.no_grad():
        m.weights.copy_(dev(case["W"])); m.biases.copy_(dev(case["b"]))
    ref = O.reference(case, "dense", "max")
    O.assert_flip_free(ref, "max")
    out = m(dev(case["q"]), dev(case["s"]), dev(case["idx"]), dev(case["f"]), case["radius"])
    O.check(dict(out=out.detach().cpu().numpy()), ref, case, "dense")
    out.backward(dev(case["go"]))
    O.close(m.weights.grad.cpu().numpy(), ref["grad_W"])


def test_options_outside_the_kernels_are_refused():
    from contrastboundary_amd import local_aggregation as LA
    case = O.base_case("dp", 1, None)
    q, s, idx, f, W, b = (dev(case[k]) for k in ("q", "s", "idx", "f", "W", "b"))
    for kw, exc, match in ((dict(local_input_feature="rscnn"), NotImplementedError, "rscnn"), (dict(local_input_feature="gac"), NotImplementedError, "gac"),
                           (dict(weight_softmax="softmax"), NotImplementedError, "weight_softmax"),
                           (dict(shared_channels=5), NotImplementedError, "shared_channels"), (dict(shared_channels=3), NotImplementedError, "shared_channels"),
                           (dict(local_input_feature="dp_fj"), ValueError, "fc_weight")):
        with pytest.raises(exc, match=match):
            LA.adaptive_weight(q, s, idx, f, 0.15, W, b, "sum", **kw)
    with pytest.raises(NotImplementedError, match="fc_num"):
        LA.AdaptiveWeight(12, fc_num=2)
    with pytest.raises(NotImplementedError):
        LA.adaptive_weight(q, s, dev(np.zeros((O.BASE[1], 129), np.int32)), f, 0.15, W, b, "max")       # K > 128
