"""GPU: the scene-segmentation head (contrastboundary_amd/seg_head.ResnetSceneSegmentationHead; tensorflow/models/heads/seg_head.py:31-102) on a five-layer toy
pyramid — rows (150, 70, 33, 17, 9), base_fdim 8 (F widths 16 .. 256), 13 classes, random upsample tables with shadow ids — in training and evaluation mode
against the float64 composition of the per-layer oracles (tests/seg_head_oracle.py; TF absent: parity unpinned by execution) within the 1e-4 contract: F_up,
features, logits, the gradient of a random cotangent on the logits with respect to every F[i] and every parameter, and the moving statistics.  The seed is
flip-free at every layer (found on the CPU, asserted here)."""
import functools

import numpy as np
import pytest
import torch

from tests import seg_head_oracle as S

pytestmark = pytest.mark.gpu
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
host = lambda t: t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference(training):
    ref = S.reference(S.make_case(S.SEED), training)
    assert ref["min_abs_z"] >= 1e-5, "bad seed: a pre-activation within 1e-5 of zero (%.2e)" % ref["min_abs_z"]
    return ref


def head(case, **kw):
    from contrastboundary_amd import seg_head
    m = seg_head.ResnetSceneSegmentationHead(S.BASE_FDIM, S.NUM_CLASSES, **kw)
    state = {"%s.%s" % (layer, name): torch.from_numpy(v) for layer, p in case["params"].items() if hasattr(m, layer) for name, v in p.items()}
    assert sorted(state) == sorted(m.state_dict())                   # the state_dict names are the reference's layer and variable names
    m.load_state_dict(state)
    return m.cuda()


@pytest.mark.parametrize("training", [True, False])
def test_against_the_float64_composition(training):
    case, ref = S.make_case(S.SEED), reference(training)
    m = head(case).train(training)
    F = [dev(f).requires_grad_(True) for f in case["F"]]
    inputs = dict(upsamples=[dev(u) for u in case["upsamples"]])
    F_up, (features, logits) = m(inputs, F)
    assert [tuple(f.shape) for f in F_up] == [(S.ROWS[i], S.WIDTHS[i] // 2) for i in range(4)]        # finest first (seg_head.py:91)
    for i, f in enumerate(F_up):
        S.O.close(host(f), ref["F_up"][i], "F_up[%d]" % i)
    S.O.close(host(features), ref["features"], "features")
    S.O.close(host(logits), ref["logits"], "logits")
    logits.backward(dev(case["go"]))
    for i, f in enumerate(F):
        S.O.close(host(f.grad), ref["grad_F"][i], "grad F[%d]" % i)
    for layer in S.LAYERS:
        for name, want in ref["grads"][layer].items():
            got, what = host(getattr(getattr(m, layer), name).grad), "grad %s.%s" % (layer, name)
            if name == "weights":
                S.O.close(got, want, what)
            else:
                S.O.close_sum(got, want, ref["totals"][layer][name], what)
    for layer in S.LAYERS[:-1]:
        for name in ("moving_mean", "moving_variance"):
            got = host(getattr(getattr(m, layer), name))
            if training:
                S.O.close(got, ref["moving"][layer][name], "%s.%s" % (layer, name))
            else:
                np.testing.assert_array_equal(got, case["params"][layer][name])       # evaluation leaves them alone


@pytest.mark.parametrize("kw", [dict(sep_head=True), dict(arch_up=True)])
def test_sep_head_and_arch_up_return_the_decoder_alone(kw):
    case, ref = S.make_case(S.SEED), reference(True)
    m = head(case, **kw).train()
    assert not hasattr(m, "segmentation_head") and not hasattr(m, "segmentation_pred")
    F_up, rest = m(dict(upsamples=[dev(u) for u in case["upsamples"]]), [dev(f) for f in case["F"]])
    assert rest is None and len(F_up) == 4
    for i, f in enumerate(F_up):
        S.O.close(host(f), ref["F_up"][i], "F_up[%d]" % i)


def test_tf_scopes_and_variables_are_the_references():
    """seg_head.py:59-101: everything under resnet_scene_segmentation_head/; up_conv* and segmentation_head without a bias and with a batch norm (variables
    under <layer>/bn), segmentation_pred with a bias and without one; ONE weights variable per up_conv of (c_up + c_skip, c_out)"""
    from contrastboundary_amd import seg_head
    m = seg_head.ResnetSceneSegmentationHead(S.BASE_FDIM, S.NUM_CLASSES)
    root = "resnet_scene_segmentation_head/"
    want = {}
    for layer in S.LAYERS[:-1]:
        want[layer + ".weights"] = root + layer
        for name in ("gamma", "beta", "moving_mean", "moving_variance"):
            want["%s.%s" % (layer, name)] = root + layer + "/bn"
    want["segmentation_pred.weights"] = want["segmentation_pred.biases"] = root + "segmentation_pred"
    assert m.tf_scopes() == want and sorted(m.state_dict()) == sorted(want)
    assert {layer: tuple(getattr(m, layer).weights.shape) for layer in S.LAYERS} == S.shapes()
    assert m.segmentation_pred.activation_fn is None
    with pytest.raises(NotImplementedError):                         # five layers, as the reference
        m.cuda()(dict(upsamples=[None] * 5), [torch.zeros(4, 16).cuda()] * 4)
