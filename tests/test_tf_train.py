"""CPU: contrastboundary_amd.tf_train without a device — which variables the reference decays (decayed_variables), by TF variable name, on a ResnetBackbone
of every aggregator kind plus the segmentation head (constructing the modules needs no device); and that CPU tensors raise.  The expected names are written
out here from the reference's graph code, not taken from the module under test:
  conv1d_1x1 / batch_conv1d_1x1 `weights`: _variable_with_weight_decay(..., wd=weight_decay)  tensorflow/models/basic_operators.py:225-228, :273-276
  PseudoGrid `weights`:                    local_aggregation_operators.py:720-723
  AdaptiveWeight's fc layers:              weight_decay=0  local_aggregation_operators.py:423, :429 — NOT decayed
  gamma, beta, biases:                     plain variables — not decayed"""
import pytest
import torch

from contrastboundary_amd import _lib, tf_train
from contrastboundary_amd.convnet_blocks import KINDS, LocalAggregation, ResnetBackbone
from contrastboundary_amd.seg_head import ResnetSceneSegmentationHead

BACKBONE, HEAD = "resnet_backbone/", "resnet_scene_segmentation_head/"


def expected_names(kind):
    """depth 1, five layers (resnet.py:344-440): the input conv; per bottleneck conv1 and conv3, and the shortcut conv where the widths differ (the first
    bottleneck of stage 1 and every strided one); per local aggregation what its kind creates with a weight decay; the head's six layers (seg_head.py:63-101)"""
    names = [BACKBONE + "res1_input_conv/weights"]
    las = [BACKBONE + "res1_simple_block/local_aggreagtion"]
    blocks = [("res1_bottleneck0", True)]
    for nl in range(2, 6):
        blocks += [("res%d_strided_bottleneck" % nl, True), ("res%d_bottleneck0" % nl, False)]
    for block, shortcut in blocks:
        names += [BACKBONE + block + "/conv1/conv1d_1x1/weights", BACKBONE + block + "/conv3/conv1d_1x1/weights"]
        if shortcut:
            names.append(BACKBONE + block + "/shortcut/conv1d_1x1/weights")
        las.append(BACKBONE + block + "/conv2/local_aggregation")
    if kind == "pointwisemlp":
        names += [la + "/fc_1/weights" for la in las]               # fc_num 1: the one layer is fc_1 (:596)
    elif kind == "pseudo_grid":
        names += [la + "/weights" for la in las]
    names += [HEAD + "up_conv%d/weights" % i for i in range(4)] + [HEAD + "segmentation_head/weights", HEAD + "segmentation_pred/weights"]
    return sorted(names)


@pytest.mark.parametrize("kind", KINDS)
def test_decayed_variables_of_backbone_and_head(kind):
    la = dict(kind=kind, **({"kernel_points": torch.randn(15, 3)} if kind == "pseudo_grid" else {}))
    backbone, head = ResnetBackbone(5, 0.1, 8, 2, 1, la), ResnetSceneSegmentationHead(8, 13)
    got = tf_train.decayed_variables(backbone, head, weight_decay=0.001)
    assert sorted(n for n, _, _ in got) == expected_names(kind)
    assert all(c == 0.001 for _, _, c in got) and all(isinstance(p, torch.nn.Parameter) for _, p, _ in got)
    every = tf_train.tf_variables(backbone, head)
    assert len(every) == len(list(backbone.parameters())) + len(list(head.parameters()))
    rest = {n for n, _, d in every if not d}
    assert all(n.rsplit("/", 1)[1] in ("gamma", "beta", "biases") or (kind == "adaptive_weight" and n.endswith("/fc_1/weights")) for n in rest), sorted(rest)[:5]
    assert tf_train.decayed_variables(backbone, head, weight_decay=0) == []             # `if wd > 0` (basic_operators.py:127)


def test_decayed_variables_of_the_deeper_per_pair_layers():
    """fc_num 2: AdaptiveWeight's fc_0 / fc_2 stay undecayed and only its output_conv is decayed; PointWiseMLP's fc_0 and fc_2 are both decayed"""
    aw = LocalAggregation(32, 64, "adaptive_weight", fc_num=2)
    assert [n for n, _, _ in tf_train.decayed_variables(aw, weight_decay=0.5)] == ["local_aggregation/output_conv/weights"]
    pw = LocalAggregation(32, 64, "pointwisemlp", fc_num=2)
    assert [n for n, _, _ in tf_train.decayed_variables(pw, weight_decay=0.5)] == ["local_aggregation/fc_0/weights", "local_aggregation/fc_2/weights"]


def test_a_module_class_nobody_read_off_the_reference_raises():
    class Foreign(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.inner = torch.nn.Linear(3, 3)

        def tf_scopes(self):
            return {"inner.weight": "x", "inner.bias": "x"}
    with pytest.raises(NotImplementedError):
        tf_train.decayed_variables(Foreign(), weight_decay=0.1)
    with pytest.raises(TypeError):
        tf_train.decayed_variables(torch.nn.Linear(3, 3), weight_decay=0.1)


def test_cpu_tensors_raise():
    from contrastboundary_amd.unary import Conv1d1x1
    with pytest.raises(_lib.CblError):
        tf_train.TFMomentum([Conv1d1x1(4, 4, scope="a")], lr=0.01)
    with pytest.raises(_lib.CblError):
        tf_train.TFMomentum([torch.nn.Parameter(torch.zeros(4))], lr=0.01)
    with pytest.raises(_lib.CblError):
        tf_train.weight_loss([torch.nn.Parameter(torch.zeros(4))], 0.1)
