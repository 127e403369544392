"""TEST ORACLE: LocalAggregation (tensorflow/models/local_aggregation_operators.py:748-863), simple_block / bottleneck / strided_bottleneck and resnet_backbone
(tensorflow/models/backbone/resnet.py:39-444) restated in torch under autograd, in the graph code's own terms: every variable is looked up by its TF NAME
(tf.variable_scope nesting + variable name, e.g. 'resnet_backbone/res1_bottleneck0/conv1/conv1d_1x1/bn/gamma'), so a module is compared through its
tf_scopes().  Composed from the aggregator oracles already in tests/ — adaptive_weight_general_oracle.direct, pointwise_mlp_oracle.direct (torch), the
geometric factors of pospool_oracle (embedding, mid_of) and kpconv_oracle (_weights, _influence) (numpy, constants of the graph) — plus batch norm in the
direct form (tests/pool_bn_oracle.py's), matmul and the two pools (tests/index_pool_oracle.py's compositions: tf.reduce_max shares a tied maximum's gradient,
torch.amax does the same).  TensorFlow itself is absent, so — as for the rest of a14 / a15 — this is a restatement only: parity is unpinned by execution.

One evaluation runs in a dtype: float64 is the reference, float32 (on the CPU, torch's own summation orders) the INDEPENDENT fp32 evaluation whose error
against the float64 one, times 4 (another summation order), is the bound for the device (tests/test_gpu_convnet_blocks.py).
Flip-free seeds: relu masks and max-pool ties make the gradient discontinuous; `Graph.guard` collects the smallest |pre-activation| (guard 1e-5, as
tests/unary_layer_oracle.py) and the smallest gap between the two largest candidates of a maximum (guard 5e-5, as
tests/adaptive_weight_general_oracle.py); seeds are chosen so that both hold (find_seed) and every case asserts them again."""
import numpy as np
import torch

from tests import adaptive_weight_general_oracle as AG
from tests import kpconv_oracle as KO
from tests import pointwise_mlp_oracle as PW
from tests import pospool_oracle as PO

GUARD_Z, GUARD_MAX = 1e-5, 5e-5
BN_VARIABLES = ("gamma", "beta", "moving_mean", "moving_variance")


class Graph:
    """the variables by TF name, the dtype of the evaluation, the mode; collects the moving-statistics updates and the two guard figures"""

    def __init__(self, variables, dtype=torch.float64, training=True, activation_fn="relu", bn_momentum=0.98, bn_eps=1e-3):
        self.dtype, self.training, self.activation_fn, self.momentum, self.eps = dtype, training, activation_fn, bn_momentum, bn_eps
        self.v = {}
        for name, a in variables.items():
            moving = name.rsplit("/", 1)[1] in ("moving_mean", "moving_variance")
            self.v[name] = torch.tensor(np.asarray(a), dtype=dtype, requires_grad=not moving)
        self.updates, self.min_abs_z, self.min_gap, self.used = {}, np.inf, np.inf, set()

    def var(self, scope, name):
        self.used.add(scope + "/" + name)
        return self.v[scope + "/" + name]

    def t(self, a, grad=False):
        a = np.asarray(a)
        return torch.tensor(a, dtype=self.dtype if a.dtype.kind == "f" else torch.int64, requires_grad=grad)

    def act(self, z, activation_fn):
        if activation_fn in ("relu", "leaky_relu"):
            if z.numel():
                self.min_abs_z = min(self.min_abs_z, float(z.detach().abs().min()))
            return torch.relu(z) if activation_fn == "relu" else torch.nn.functional.leaky_relu(z, 0.2)
        return z

    def gap(self, cand, keep=None, positive_only=False):
        """cand (n, K, C): the candidates of a maximum over K; keep (n, K) bool: the entries that count (one per distinct source); positive_only: a
        maximum of relu outputs that is 0 is attained by every non-positive candidate at once and carries no gradient (tests/pointwise_mlp_oracle.py's rule)"""
        c = cand.detach()
        if keep is not None:
            c = torch.where(keep[..., None], c, torch.full_like(c, -np.inf))
        if c.shape[1] > 1 and c.numel():
            top = c.topk(2, dim=1).values
            g = top[:, 0] - top[:, 1]
            # an EXACT tie is no hazard: it is one of relu's exact zeros (whose sign the |z| guard pins) on both sides, and the gradient's share
            # among tied entries is the pools' documented rule; a gap inside (0, GUARD_MAX) is one
            g = g[torch.isfinite(g) & (g > 0) & ((top[:, 0] > 0) | (not positive_only))]
            if g.numel():
                self.min_gap = min(self.min_gap, float(g.min()))

    def guarded(self):
        return self.min_abs_z >= GUARD_Z and self.min_gap >= GUARD_MAX


def batch_norm(g, x, scope, bn=True):
    """basic_operators.batch_norm = tf.layers.batch_normalization(name=scope): biased batch variance, moving = moving * momentum + batch * (1 - momentum)"""
    if not bn:
        return x
    gamma, beta, mm, mv = (g.var(scope, n) for n in BN_VARIABLES)
    if g.training:
        mean, var = x.mean(0), x.var(0, unbiased=False)
        g.updates[scope + "/moving_mean"] = (mm * g.momentum + mean * (1 - g.momentum)).detach()
        g.updates[scope + "/moving_variance"] = (mv * g.momentum + var * (1 - g.momentum)).detach()
    else:
        mean, var = mm, mv
    return (x - mean) / torch.sqrt(var + g.eps) * gamma + beta


def conv1d_1x1(g, x, scope, activation_fn, bn=True, shortcut=None):
    """basic_operators.py:195-241; shortcut: added before the activation (resnet.py:187-192)"""
    x = batch_norm(g, x @ g.var(scope, "weights"), scope + "/bn", bn)
    if shortcut is not None:
        x = x + shortcut
    return g.act(x, activation_fn)


def _row_ids(inds, n1):
    return torch.where((inds >= 0) & (inds < n1), inds, torch.full_like(inds, n1))


def _first_of_each_id(ids):
    """(n, K) bool: False on an entry whose id already occurred in its row (a shadow id repeated: one candidate, not a tie)"""
    a = ids.numpy()
    keep = np.ones(a.shape, bool)
    for j in range(1, a.shape[1]):
        keep[:, j] = (a[:, :j] != a[:, j:j + 1]).all(1)
    return torch.from_numpy(keep)


def ind_max_pool(g, x, inds):
    """basic_operators.py:155-172: the shadow row is the column minimum"""
    ids = _row_ids(inds, x.shape[0])
    v = torch.cat([x, x.amin(0, keepdim=True)])[ids]
    g.gap(v, _first_of_each_id(ids))
    return v.amax(1)


def ind_closest_pool(g, x, inds):
    return torch.cat([x, torch.zeros_like(x[:1])])[_row_ids(inds, x.shape[0])[:, 0]]


def _reduce(g, a, idx, n0, reduction):
    """the reductions PosPool and AdaptiveWeight share (:212-230, :462-480)"""
    if reduction == "max":
        cand = a + (idx >= n0).to(a.dtype)[..., None] * -65535.0
        g.gap(cand)
        return cand.amax(1)
    out = a.sum(1)
    if reduction in ("mean", "avg"):
        out = out / ((idx < idx.max()).to(a.dtype).sum(-1, keepdim=True) + 1e-5)
    return out


def LocalAggregation(g, kind, options, q, s, idx, f, scope, radius, out_fdim, bn=True):
    """:748-863.  q, s, idx: numpy; f: tensor (n0, fdim)"""
    opt = dict(options)
    act = g.activation_fn
    fdim, n0 = f.shape[1], s.shape[0]
    tq, ts, tidx = g.t(q), g.t(s), g.t(idx)
    gather = lambda x: torch.cat([x, torch.zeros_like(x[:1])])[_row_ids(tidx, n0)]
    if kind == "pointwisemlp":                                       # :503-614, fc_num 1
        assert opt.get("fc_num", 1) == 1
        sc = scope + "/fc_1"
        training = "batch" if g.training else "moving"
        gamma, beta, mm, mv = (g.var(sc, n) for n in BN_VARIABLES) if bn else (None,) * 4
        out, z, a, mean, var = PW.direct(tq, ts, tidx, f, g.var(sc, "weights"), gamma, beta, radius, opt.get("local_input_feature", "dp_fj"),
                                         opt.get("reduction", "max"), act, training if bn else None, mm, mv, g.eps)
        if bn and g.training:
            g.updates[sc + "/moving_mean"] = (mm * g.momentum + mean * (1 - g.momentum)).detach()
            g.updates[sc + "/moving_variance"] = (mv * g.momentum + var * (1 - g.momentum)).detach()
        real = tidx < n0
        if act in ("relu", "leaky_relu") and bool(real.any()):
            g.min_abs_z = min(g.min_abs_z, float(z.detach()[real].abs().min()))
        if opt.get("reduction", "max") == "max":
            g.gap(a, positive_only=True)
        return out
    if kind == "identity":                                           # :252-313
        x = ind_closest_pool(g, f, tidx)
        if fdim != out_fdim:
            return conv1d_1x1(g, x, scope + "/output_conv", act, bn)
        return g.act(batch_norm(g, x, scope + "/pool_bn", bn), act)
    if kind == "adaptive_weight":                                    # :316-500, fc_num 1
        assert opt.get("fc_num", 1) == 1
        S = min(opt.get("shared_channels", 1), fdim)
        # (direct's 'sum' returns the products before the reduction as well; the reduction itself is _reduce, which records the gap of a maximum)
        _, a = AG.direct(tq, ts, tidx, f, g.var(scope + "/fc_1", "weights"), g.var(scope + "/fc_1", "biases"), radius, opt.get("local_input_feature", "dp"), S,
                         opt.get("weight_softmax", False), "sum")
        x = _reduce(g, a, tidx, n0, opt.get("reduction", "mean"))
        bn_scope = scope + "/pool_bn"
    elif kind == "pospool":                                          # :15-249
        pe = opt.get("position_embedding", "sin_cos")
        # the normalised offsets in the evaluation's dtype (the shadow point is the origin), the embedding by the PosPool oracle's own function
        rel = ((gather(ts) - tq[:, None, :]) / float(radius)).numpy()
        mid = PO.mid_of(pe, fdim)
        assert mid > 0
        geo = g.t(np.repeat(PO.embedding(rel, pe, fdim), fdim // mid, axis=-1))      # (n, K, fdim): channel c takes entry c // shared
        x = _reduce(g, geo * gather(f), tidx, n0, opt.get("reduction", "mean"))
        bn_scope = scope + "/pool_bn"
    elif kind == "pseudo_grid":                                      # :617-745
        extent = float(opt.get("KP_extent", 1.0)) * float(radius) / float(opt.get("density_parameter", 5.0))
        kpts = np.asarray(opt["kernel_points"], np.float32)
        # kpconv_oracle._weights / _influence restated in the evaluation's dtype (those two compute in float64 whatever they are given): squared distances
        # neighbour - centre - kernel point with the shadow point at 1e6, then the influence
        real = (tidx >= 0) & (tidx < n0)
        nb = torch.where(real[..., None], ts[torch.where(real, tidx, torch.zeros_like(tidx))], torch.full_like(ts[:1], 1e6)) - tq[:, None, :]
        diff = nb[:, :, None, :] - g.t(kpts)[None, None]
        sq = (diff * diff).sum(-1)
        if g.dtype == torch.float64:                                  # ... which in float64 IS the KPConv oracle's
            assert np.array_equal(sq.numpy(), KO._weights(q, s, idx, kpts, slice(0, idx.shape[0]))[1])
        w = g.t(KO._influence(sq.numpy(), extent, opt.get("KP_influence", "linear"), opt.get("convolution_mode", "sum")).astype(sq.numpy().dtype))      # (n, K, KP)
        wf = w.transpose(1, 2) @ gather(f)                           # (n, KP, fdim)  :717
        x = (g.var(scope, "weights")[None] * wf).sum(1)              # :725-728
        bn_scope = scope + "/bn"
    else:
        raise NotImplementedError(kind)
    x = g.act(batch_norm(g, x, bn_scope, bn), act)
    if fdim != out_fdim or opt.get("output_conv", False):
        x = conv1d_1x1(g, x, scope + "/output_conv", act, bn)
    return x


def simple_block(g, layer_ind, la, inputs, features, scope, radius, out_fdim):
    """resnet.py:39-89"""
    kind, options = la["kind"], {k: v for k, v in la.items() if k != "kind"}
    p = inputs["points"][layer_ind]
    return LocalAggregation(g, kind, options, p, p, inputs["neighbors"][layer_ind], features, scope + "/local_aggreagtion", radius, out_fdim)


def bottleneck(g, layer_ind, la, inputs, features, scope, radius, out_fdim, bottleneck_ratio, strided=False):
    """resnet.py:92-194 and, strided, :197-304"""
    kind, options = la["kind"], {k: v for k, v in la.items() if k != "kind"}
    act = g.activation_fn
    mid = out_fdim // bottleneck_ratio
    x = conv1d_1x1(g, features, scope + "/conv1/conv1d_1x1", act)
    if strided:
        q, s, idx = inputs["points"][layer_ind + 1], inputs["points"][layer_ind], inputs["pools"][layer_ind]
        shortcut = ind_max_pool(g, features, g.t(idx))
    else:
        q = s = inputs["points"][layer_ind]
        idx = inputs["neighbors"][layer_ind]
        shortcut = features
    x = LocalAggregation(g, kind, options, q, s, idx, x, scope + "/conv2/local_aggregation", radius, mid)
    if shortcut.shape[1] != out_fdim:
        shortcut = conv1d_1x1(g, shortcut, scope + "/shortcut/conv1d_1x1", None)
    return conv1d_1x1(g, x, scope + "/conv3/conv1d_1x1", act, shortcut=shortcut)


def resnet_backbone(g, la, inputs, features, base_radius, base_fdim, bottleneck_ratio, depth, num_layers=5):
    """resnet.py:307-444, num_layers 5 (the reference's own loop unrolled there) and its tail"""
    sc = "resnet_backbone"
    fdim, radius = base_fdim, base_radius
    F = []
    features = conv1d_1x1(g, features, sc + "/res1_input_conv", g.activation_fn)
    features = simple_block(g, 0, la, inputs, features, sc + "/res1_simple_block", radius, fdim)
    for i in range(depth):
        features = bottleneck(g, 0, la, inputs, features, sc + "/res1_bottleneck%d" % i, radius, 2 * fdim, bottleneck_ratio)
    for stage, (r_strided, r_block, mult) in enumerate(((1, 2, 4), (2, 4, 8), (4, 8, 16), (8, 16, 32)), 2):
        F.append(features)
        features = bottleneck(g, stage - 2, la, inputs, features, sc + "/res%d_strided_bottleneck" % stage, r_strided * radius, mult * fdim, bottleneck_ratio, True)
        for i in range(depth):
            features = bottleneck(g, stage - 1, la, inputs, features, sc + "/res%d_bottleneck%d" % (stage, i), r_block * radius, mult * fdim, bottleneck_ratio)
    for nl in range(6, num_layers + 1):
        F.append(features)
        layer_idx = nl - 1
        features = bottleneck(g, layer_idx - 1, la, inputs, features, sc + "/res%d_strided_bottleneck" % nl, (layer_idx - 1) ** 2 * radius, 2 ** nl * fdim,
                              bottleneck_ratio, True)
        for i in range(depth):
            features = bottleneck(g, layer_idx, la, inputs, features, sc + "/res%d_bottleneck%d" % (nl, i), layer_idx ** 2 * radius, 2 ** nl * fdim,
                                  bottleneck_ratio)
    F.append(features)
    return F


# ---------------------------------------------------------------------------------------------------------------- cases
def tf_variables(module, tf_scopes=None):
    """a module's state_dict under TF names: tf_scopes()[key] + '/' + the variable's own name (the key's last component)"""
    scopes = module.tf_scopes() if tf_scopes is None else tf_scopes
    out = {}
    for key, value in module.state_dict().items():
        name = scopes[key] + "/" + key.rsplit(".", 1)[-1]
        assert name not in out, "two variables named " + name
        out[name] = value.detach().cpu().numpy().copy()
    return out


def randomize_(module, seed):
    """every variable of a freshly built module off its initial value, from one seed: weights as drawn times a factor near 1, gamma in [0.5, 1.5], beta and
    the moving means ~ N(0, 0.3), the moving variances in [0.5, 1.5], biases ~ N(0, 0.3)"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for key, v in module.state_dict().items():
            name = key.rsplit(".", 1)[-1]
            r = torch.rand(v.shape, generator=gen)
            nrm = torch.randn(v.shape, generator=gen)
            if name in ("gamma", "moving_variance"):
                v.copy_(0.5 + r)
            elif name in ("beta", "moving_mean") or name.startswith("biases"):
                v.copy_(0.3 * nrm)
            else:
                v.copy_(nrm / float(v.shape[0]) ** 0.5)


def evaluate(build, variables, inputs, features, go, dtype=torch.float64, training=True, backward=True, **graph_options):
    """build(g, features) -> tensor or list of tensors; go: matching cotangent(s).  -> dict(out=[...], grad_features, grads {TF name: array}, updates
    {TF name: array}, guarded, min_abs_z, min_gap, used)"""
    g = Graph(variables, dtype, training, **graph_options)
    f = g.t(features, True)
    out = build(g, f)
    outs = list(out) if isinstance(out, (list, tuple)) else [out]
    gos = go if isinstance(go, (list, tuple)) else [go]
    if not backward:                                                 # the seed search: the guard figures are the forward pass's
        return dict(guarded=g.guarded(), min_abs_z=g.min_abs_z, min_gap=g.min_gap, updates={k: v.double().numpy() for k, v in g.updates.items()})
    torch.autograd.backward(outs, [g.t(c) for c in gos])
    f64 = lambda a: a.detach().double().numpy()
    return dict(out=[f64(o) for o in outs], grad_features=f64(f.grad), grads={k: f64(v.grad) for k, v in g.v.items() if v.requires_grad and v.grad is not None},
                updates={k: f64(v) for k, v in g.updates.items()}, guarded=g.guarded(), min_abs_z=g.min_abs_z, min_gap=g.min_gap, used=g.used)


def flat(r):
    """the tensors of an evaluation under one set of keys: out0.., grad_features, 'grad <TF name>', 'update <TF name>'"""
    return dict([("out%d" % i, o) for i, o in enumerate(r["out"])] + [("grad_features", r["grad_features"])] +
                [("grad " + k, v) for k, v in r["grads"].items()] + [("update " + k, v) for k, v in r["updates"].items()])


def error_figure(got, ref):
    """THE error of a set of tensors against the reference: the worst, over every tensor and every entry, |got - ref| / scale of that tensor, scale =
    max|ref of that tensor|.  A tensor whose reference is ZERO in exact arithmetic has no scale of its own (the backbone has one: at its last stage every
    point is a neighbour of every point, the bias of the aggregation's FC layer shifts every row alike, the batch norm behind it removes the shift and the
    bias gradient is 1e-22 in float64, while its terms are of the size of the other gradients and cancel): a tensor whose largest entry is below one
    float32 unit (2^-23) of the largest tensor of its kind (outputs / gradients / updated buffers) is zero to float32 working precision, what any fp32
    evaluation returns for it is the rounding noise of those terms, and it is measured against that largest tensor's scale.  -> (figure, the key that
    attains it)"""
    assert got.keys() == ref.keys(), sorted(got.keys() ^ ref.keys())
    kind = lambda k: "out" if k.startswith("out") else "update" if k.startswith("update") else "grad"
    largest = {}
    for k in ref:
        if ref[k].size:
            largest[kind(k)] = max(largest.get(kind(k), 0.0), float(np.abs(ref[k]).max()))
    worst, where = 0.0, None
    for k in ref:
        if ref[k].size:
            g = np.asarray(got[k], np.float64)
            scale = float(np.abs(ref[k]).max())
            if scale < 2.0 ** -23 * largest[kind(k)]:
                scale = largest[kind(k)]
            scale = max(scale, 1e-30)
            e = float(np.abs(g - ref[k]).max()) / scale if np.isfinite(g).all() else np.inf
            if e >= worst:
                worst, where = e, k
    return worst, where
