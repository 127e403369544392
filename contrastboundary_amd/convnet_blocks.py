"""The ConvNet's ResNet backbone (tensorflow/models/backbone/resnet.py:39-444) and the LocalAggregation dispatcher under it
(tensorflow/models/local_aggregation_operators.py:748-863) as modules over the library's operators: an aggregator of local_aggregation.py,
then pool_bn (unary.pool_bn: TF batch norm + activation, csrc/pool_bn.hip), then output_conv (unary.Conv1d1x1).  Nothing here is a kernel: every step is
one of the library's entries under autograd, and there is no fallback — CPU tensors raise in the operator that meets them.

Every module carries the reference's variable names and tf_scopes(): state_dict key -> the tf.variable_scope nesting of that variable, so that a reference
checkpoint's names map one to one (TensorFlow is absent here: the scopes are read off the graph code, tests/test_gpu_convnet_blocks.py lists them by hand).
`inputs` is the pyramid of tf_ops.segmentation_inputs_radius: inputs['points'][l], inputs['neighbors'][l], inputs['pools'][l]."""
import torch

from . import local_aggregation as LA
from .unary import Conv1d1x1, PoolBN

KINDS = ("pospool", "adaptive_weight", "pointwisemlp", "pseudo_grid", "identity")


def _join(*scopes):
    return "/".join(s for s in scopes if s)


def _scoped(module, children, scope):
    """state_dict key -> TF scope of a composite: every child's own tf_scopes() under the composite's scope"""
    names = {}
    for attr in children:
        child = getattr(module, attr, None)
        if child is not None:
            for key, sc in child.tf_scopes().items():
                names[attr + "." + key] = _join(scope, sc)
    return names


class _KPConvWeights(torch.nn.Module):
    """PseudoGrid's variable `weights` (num_kernel_points, fdim) (local_aggregation_operators.py:720-723) and its constant kernel points"""

    def __init__(self, fdim, kernel_points, init):
        super().__init__()
        if not (isinstance(kernel_points, torch.Tensor) and kernel_points.dim() == 2 and kernel_points.shape[1] == 3):
            raise ValueError("pseudo_grid: kernel_points (num_kernel_points, 3) expected (a tensor: their generator is not part of the library)")
        self.register_buffer("kernel_points", kernel_points.detach().to(torch.float32).contiguous().clone(), persistent=False)
        self.weights = torch.nn.Parameter(torch.empty(kernel_points.shape[0], fdim))
        if init == "xavier":
            torch.nn.init.xavier_uniform_(self.weights)
        elif init == "fan_in":
            LA.fan_in_init_(self.weights)
        else:
            raise NotImplementedError("pseudo_grid: init {} ('xavier' or 'fan_in')".format(init))

    def tf_scopes(self):
        return {"weights": ""}


class LocalAggregation(torch.nn.Module):
    """LocalAggregation(config, ...) of local_aggregation_operators.py:748-863 for one (in_fdim, out_fdim): `kind` is config.local_aggreagtion, the keyword
    options are config.<kind>.* (and config.density_parameter for pseudo_grid) as the operators of local_aggregation.py document them — what they reject
    stays rejected.
      'adaptive_weight' : local_input_feature, shared_channels, fc_num, weight_softmax, reduction, output_conv    (:316-500)
      'pospool'         : position_embedding, reduction, output_conv                                              (:15-249)
      'pseudo_grid'     : kernel_points (a tensor (K, 3), already at K_radius = 1.5 extent), KP_influence, KP_extent, convolution_mode, density_parameter,
                          output_conv                                                                             (:617-745)
        each: aggregator -> pool_bn (scope 'pool_bn'; 'bn' for pseudo_grid) -> activation -> output_conv iff in_fdim != out_fdim or output_conv
      'identity'        : ind_closest_pool, then output_conv if in_fdim != out_fdim, else pool_bn                 (:252-313)
      'pointwisemlp'    : local_input_feature, fc_num, reduction — a straight dispatch, its batch norms live inside the operator   (:503-614)
    'attention_point' is not implemented."""

    def __init__(self, in_fdim, out_fdim, kind, scope="local_aggregation", init="xavier", activation_fn="relu", bn=True, bn_momentum=0.98, bn_eps=1e-3,
                 **options):
        super().__init__()
        if kind in ("attention", "attention_point"):
            raise NotImplementedError("local_aggreagtion {}: not part of the library".format(kind))
        if kind not in KINDS:
            raise NotImplementedError("Local aggregation {} not supported (one of {})".format(kind, ", ".join(KINDS)))
        self.kind, self.in_fdim, self.out_fdim, self.scope = kind, in_fdim, out_fdim, scope
        opt = dict(options)
        take = lambda name, default: opt.pop(name, default)
        output_conv = bool(take("output_conv", False)) if kind in ("adaptive_weight", "pospool", "pseudo_grid") else False
        common = dict(activation_fn=activation_fn, bn=bn, bn_momentum=bn_momentum, bn_eps=bn_eps)
        self.aggregator = self.pool_bn = self.output_conv = None
        if kind == "adaptive_weight":
            self.aggregator = LA.AdaptiveWeight(in_fdim, take("local_input_feature", "dp"), take("shared_channels", 1), take("fc_num", 1),
                                                take("weight_softmax", False), take("reduction", "mean"), activation_fn)
        elif kind == "pospool":
            self.position_embedding, self.reduction = take("position_embedding", "sin_cos"), take("reduction", "mean")
            if self.position_embedding not in LA.POSPOOL_EMBEDDINGS:
                raise NotImplementedError("position_embedding [{}] not supported in PosPool ".format(self.position_embedding))
            if self.reduction not in LA._POSPOOL_REDUCTIONS:
                raise NotImplementedError("Reduction {} not supported in PosPool".format(self.reduction))
        elif kind == "pseudo_grid":
            self.KP_influence, self.convolution_mode = take("KP_influence", "linear"), take("convolution_mode", "sum")
            self.KP_extent, self.density_parameter = float(take("KP_extent", 1.0)), float(take("density_parameter", 5.0))
            if self.KP_influence not in ("linear", "constant"):
                raise NotImplementedError("KP_influence 'gaussian': radius_gaussian is not defined in the reference")
            if self.convolution_mode not in ("sum", "closest"):
                raise ValueError("Unknown convolution mode. Should be 'closest' or 'sum'")
            self.aggregator = _KPConvWeights(in_fdim, take("kernel_points", None), init)
        elif kind == "pointwisemlp":
            self.aggregator = LA.PointWiseMLP(in_fdim, out_fdim, take("local_input_feature", "dp_fj"), take("fc_num", 1), take("reduction", "max"), **common)
        if opt:
            raise TypeError("LocalAggregation {}: unknown options {}".format(kind, sorted(opt)))
        if kind in ("adaptive_weight", "pospool", "pseudo_grid"):
            self.pool_bn = PoolBN(in_fdim, scope="bn" if kind == "pseudo_grid" else "pool_bn", **common)
            if in_fdim != out_fdim or output_conv:
                # (PseudoGrid's output_conv is built without bn_momentum / bn_eps, :740-743: conv1d_1x1's defaults, which are the same numbers)
                conv = common if kind != "pseudo_grid" else dict(activation_fn=activation_fn, bn=bn)
                self.output_conv = Conv1d1x1(in_fdim, out_fdim, init=init, scope="output_conv", **conv)
        elif kind == "identity":
            if in_fdim != out_fdim:
                self.output_conv = Conv1d1x1(in_fdim, out_fdim, init=init, scope="output_conv", **common)
            else:
                self.pool_bn = PoolBN(in_fdim, scope="pool_bn", **common)

    def tf_scopes(self):
        return _scoped(self, ("aggregator", "pool_bn", "output_conv"), self.scope)

    def forward(self, query_points, support_points, neighbors_indices, features, radius):
        if features.dim() != 2 or features.shape[1] != self.in_fdim:
            raise ValueError("LocalAggregation: features of shape {}, (n0, {}) expected".format(tuple(features.shape), self.in_fdim))
        if self.kind == "pointwisemlp":
            return self.aggregator(query_points, support_points, neighbors_indices, features, radius)
        if self.kind == "identity":
            x = LA.ind_closest_pool(features, neighbors_indices)
            return self.output_conv(x) if self.output_conv is not None else self.pool_bn(x)
        if self.kind == "adaptive_weight":
            x = self.aggregator(query_points, support_points, neighbors_indices, features, radius)
        elif self.kind == "pospool":
            x = LA.pospool(query_points, support_points, neighbors_indices, features, radius, self.position_embedding, self.reduction)
        else:
            extent = self.KP_extent * float(radius) / self.density_parameter                # :664
            x = LA.kpconv(query_points, support_points, neighbors_indices, features, self.aggregator.kernel_points, self.aggregator.weights, extent,
                          self.KP_influence, self.convolution_mode)
        x = self.pool_bn(x)
        return self.output_conv(x) if self.output_conv is not None else x


def _la_options(la):
    la = dict(la)
    if "kind" not in la:
        raise TypeError("the local aggregation's options need 'kind' (config.local_aggreagtion)")
    return la.pop("kind"), la


class SimpleBlock(torch.nn.Module):
    """simple_block (resnet.py:39-89): one LocalAggregation of layer `layer_ind` on itself.  la: dict(kind=..., the kind's options)"""

    def __init__(self, layer_ind, in_fdim, out_fdim, radius, la, scope="", **common):
        super().__init__()
        kind, options = _la_options(la)
        self.layer_ind, self.radius, self.scope = layer_ind, float(radius), scope
        self.local_aggreagtion = LocalAggregation(in_fdim, out_fdim, kind, scope="local_aggreagtion", **common, **options)      # (sic: :79)

    def tf_scopes(self):
        return _scoped(self, ("local_aggreagtion",), self.scope)

    def forward(self, inputs, features):
        l = self.layer_ind
        return self.local_aggreagtion(inputs["points"][l], inputs["points"][l], inputs["neighbors"][l], features, self.radius)


class Bottleneck(torch.nn.Module):
    """bottleneck (resnet.py:92-194): conv1 -> LocalAggregation -> conv3 + shortcut -> activation.  conv3, the shortcut's add and the activation are ONE
    conv1d_1x1(..., shortcut=...) call (unary.conv1d_1x1: act(bn(x @ w) + shortcut)); the shortcut is a bn'd conv1d_1x1 without activation when the widths
    differ, the features themselves when not.  `strided` (strided_bottleneck, :197-304): the aggregation runs query = points[l + 1], support = points[l],
    indices = pools[l], and the shortcut is ind_max_pool(features, pools[l]) first."""

    def __init__(self, layer_ind, in_fdim, out_fdim, bottleneck_ratio, radius, la, scope="", strided=False, init="xavier", activation_fn="relu", bn=True,
                 bn_momentum=0.98, bn_eps=1e-3):
        super().__init__()
        kind, options = _la_options(la)
        if out_fdim is None:
            out_fdim = in_fdim
        mid = out_fdim // bottleneck_ratio
        if mid < 1:
            raise ValueError("bottleneck: out_fdim {} // bottleneck_ratio {} leaves no width".format(out_fdim, bottleneck_ratio))
        self.layer_ind, self.radius, self.scope, self.strided = layer_ind, float(radius), scope, strided
        common = dict(init=init, bn=bn, bn_momentum=bn_momentum, bn_eps=bn_eps)
        self.conv1 = Conv1d1x1(in_fdim, mid, activation_fn=activation_fn, scope="conv1/conv1d_1x1", **common)
        self.conv2 = LocalAggregation(mid, mid, kind, scope="conv2/local_aggregation", activation_fn=activation_fn, **common, **options)
        self.conv3 = Conv1d1x1(mid, out_fdim, activation_fn=activation_fn, scope="conv3/conv1d_1x1", **common)     # (the activation follows the shortcut's add)
        self.shortcut = Conv1d1x1(in_fdim, out_fdim, activation_fn=None, scope="shortcut/conv1d_1x1", **common) if in_fdim != out_fdim else None

    def tf_scopes(self):
        return _scoped(self, ("conv1", "conv2", "conv3", "shortcut"), self.scope)

    def forward(self, inputs, features):
        l = self.layer_ind
        x = self.conv1(features)
        if self.strided:
            x = self.conv2(inputs["points"][l + 1], inputs["points"][l], inputs["pools"][l], x, self.radius)
            shortcut = LA.ind_max_pool(features, inputs["pools"][l])
        else:
            x = self.conv2(inputs["points"][l], inputs["points"][l], inputs["neighbors"][l], x, self.radius)
            shortcut = features
        if self.shortcut is not None:
            shortcut = self.shortcut(shortcut)
        return self.conv3(x, shortcut=shortcut)


class StridedBottleneck(Bottleneck):
    """strided_bottleneck (resnet.py:197-304): layer_ind is the layer of the support points, layer_ind + 1 that of the query points"""

    def __init__(self, layer_ind, in_fdim, out_fdim, bottleneck_ratio, radius, la, scope="", **common):
        super().__init__(layer_ind, in_fdim, out_fdim, bottleneck_ratio, radius, la, scope, strided=True, **common)


class ResnetBackbone(torch.nn.Module):
    """resnet_backbone (resnet.py:307-444): res1_input_conv, res1_simple_block, `depth` bottlenecks per stage, a strided bottleneck between stages; returns
    the list F of every stage's features (widths 2, 4, 8, ... times base_fdim).  num_layers 5, or more: the reference's tail (:423-440), whose radii are
    (layer_idx - 1)^2 and layer_idx^2 times base_radius and whose widths are 2^nl base_fdim — mirrored as they are.
    la: dict(kind=config.local_aggreagtion, the kind's options); for 'pseudo_grid' its kernel_points are those of K_radius = 1 and are scaled by every
    block's K_radius = 1.5 KP_extent radius / density_parameter (:664-665)."""

    def __init__(self, in_fdim, base_radius, base_fdim, bottleneck_ratio, depth, la, num_layers=5, init="xavier", activation_fn="relu", bn=True,
                 bn_momentum=0.98, bn_eps=1e-3):
        super().__init__()
        if num_layers < 5:
            raise NotImplementedError("unsupported num_layers = {} in resnet backbone".format(num_layers))
        common = dict(init=init, activation_fn=activation_fn, bn=bn, bn_momentum=bn_momentum, bn_eps=bn_eps)
        self.scope, self.num_layers, self.depth = "resnet_backbone", num_layers, depth
        fdim, radius = base_fdim, float(base_radius)

        def la_at(r):
            if la.get("kind") != "pseudo_grid":
                return la
            if not isinstance(la.get("kernel_points"), torch.Tensor):
                raise ValueError("pseudo_grid: kernel_points (num_kernel_points, 3) of K_radius = 1 expected (a tensor: their generator is not part of the library)")
            k_radius = 1.5 * float(la.get("KP_extent", 1.0)) * r / float(la.get("density_parameter", 5.0))
            return dict(la, kernel_points=la["kernel_points"] * k_radius)

        self.res1_input_conv = Conv1d1x1(in_fdim, fdim, scope="res1_input_conv", **common)
        self.res1_simple_block = SimpleBlock(0, fdim, fdim, radius, la_at(radius), scope="res1_simple_block", **common)
        self.order = ["res1_input_conv", "res1_simple_block"]       # the blocks in the order they run; stage_end: those whose output enters F
        self.stage_end = []
        width = fdim

        def add(name, block):
            setattr(self, name, block)
            self.order.append(name)

        for i in range(depth):
            add("res1_bottleneck%d" % i, Bottleneck(0, width, 2 * fdim, bottleneck_ratio, radius, la_at(radius), scope="res1_bottleneck%d" % i, **common))
            width = 2 * fdim
        for nl in range(2, num_layers + 1):
            self.stage_end.append(self.order[-1])
            layer_idx = nl - 1
            if nl <= 5:
                r_strided, r_block, out = 2 ** (nl - 2) * radius, 2 ** (nl - 1) * radius, 2 ** nl * fdim
            else:
                r_strided, r_block, out = (layer_idx - 1) ** 2 * radius, layer_idx ** 2 * radius, 2 ** nl * fdim
            add("res%d_strided_bottleneck" % nl, StridedBottleneck(layer_idx - 1, width, out, bottleneck_ratio, r_strided, la_at(r_strided),
                                                                   scope="res%d_strided_bottleneck" % nl, **common))
            width = out
            for i in range(depth):
                add("res%d_bottleneck%d" % (nl, i), Bottleneck(layer_idx, width, out, bottleneck_ratio, r_block, la_at(r_block),
                                                               scope="res%d_bottleneck%d" % (nl, i), **common))
        self.stage_end.append(self.order[-1])

    def tf_scopes(self):
        return _scoped(self, self.order, self.scope)

    def forward(self, inputs, features):
        F = []
        for name in self.order:
            block = getattr(self, name)
            features = block(features) if name == "res1_input_conv" else block(inputs, features)
            if name in self.stage_end:
                F.append(features)
        return F
