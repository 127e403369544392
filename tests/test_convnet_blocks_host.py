"""CPU: LocalAggregation, simple_block / bottleneck / strided_bottleneck and ResnetBackbone (contrastboundary_amd/convnet_blocks.py) on the WHOLE library
compiled for the host with wave semantics — the driver of tests/test_gpu_convnet_blocks.py (the same cases, seeds rule, oracle and bound) with the package's
own autograd functions and modules running on CPU tensors over the host library (tests/host_emul/host_mirror.py).  The pyramid is cbl_pyramid on the host.
A composition or scope regression shows here, on a machine without the device.  The backbone's layer sizes (every layer keeps at least 8 points) are checked
here as well, through the host library."""
import numpy as np
import pytest

from tests import test_gpu_convnet_blocks as T
from tests.host_emul import host_mirror


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("name", sorted(T.CASES))
def test_blocks_on_the_host_library(name, training):
    with host_mirror.mirror():
        T.check_block(name, training, source="host")


def test_the_backbones_pyramid_keeps_at_least_8_points_in_every_layer():
    _, host = T.pyramid(T.BB["n"], T.BB["layers"], T.BB["dl0"], clustered=True, source="host")
    sizes = [p.shape[0] for p in host["points"]]
    assert len(sizes) == 5 and sizes[0] == T.BB["n"] and min(sizes) >= 8 and sizes == sorted(sizes, reverse=True), sizes
    for l in range(5):                                               # tables of every layer index their own support layer (shadow id = its size)
        assert host["neighbors"][l].shape[0] == sizes[l] and 0 <= host["neighbors"][l].min() and host["neighbors"][l].max() <= sizes[l]
    for l in range(4):
        assert host["pools"][l].shape[0] == sizes[l + 1] and host["pools"][l].max() <= sizes[l]


@pytest.mark.parametrize("training", [True, False])
def test_backbone_on_the_host_library(training):
    with host_mirror.mirror():
        T.check_backbone(training, source="host")


def test_a_pseudo_grid_backbone_scales_unit_kernel_points_and_refuses_none():
    """ResnetBackbone takes PseudoGrid's kernel points at K_radius = 1 and hands every block those of ITS K_radius = 1.5 KP_extent radius / density_parameter
    (local_aggregation_operators.py:664-665); LocalAggregation takes them as they are.  Without them: ValueError, as LocalAggregation raises"""
    import torch
    from contrastboundary_amd import convnet_blocks as B
    unit = torch.from_numpy(T.kernel_points())
    la = dict(kind="pseudo_grid", kernel_points=unit, KP_extent=1.2, density_parameter=5.0)
    m = B.ResnetBackbone(4, 0.1, 8, 2, 1, la)
    for name, radius in (("res1_simple_block", 0.1), ("res2_strided_bottleneck", 0.1), ("res2_bottleneck0", 0.2), ("res5_bottleneck0", 1.6)):
        block = getattr(m, name)
        agg = (block.local_aggreagtion if name == "res1_simple_block" else block.conv2).aggregator
        assert block.radius == pytest.approx(radius)
        np.testing.assert_allclose(agg.kernel_points.numpy(), unit.numpy() * (1.5 * 1.2 * radius / 5.0), rtol=1e-6)
    scopes = m.tf_scopes()
    assert set(scopes) == set(m.state_dict()) and scopes["res2_bottleneck0.conv2.aggregator.weights"] == "resnet_backbone/res2_bottleneck0/conv2/local_aggregation"
    assert scopes["res2_bottleneck0.conv2.pool_bn.gamma"] == "resnet_backbone/res2_bottleneck0/conv2/local_aggregation/bn"
    with pytest.raises(ValueError):
        B.ResnetBackbone(4, 0.1, 8, 2, 1, dict(kind="pseudo_grid"))
    with pytest.raises(ValueError):
        B.LocalAggregation(24, 24, "pseudo_grid")
