"""The ConvNet's unary layer conv1d_1x1 (tensorflow/models/basic_operators.py:195-241): matmul in TF's (in, out) weight order, optional bias, TF batch norm
(biased variance, moving = moving * momentum + batch * (1 - momentum)), an optional shortcut added before the activation (the tail of a bottleneck,
backbone/resnet.py:158-192), relu / leaky_relu(0.2) / none — the two entries of csrc/unary_layer.hip (cbl_amd.h, a15 conv1d_1x1) under autograd.  There is no
fallback: CPU tensors raise, widths past 4096 raise.
up_conv / UpConv1d1x1: one decoder step of the segmentation head (models/heads/seg_head.py:63-67), nearest upsample + concat + conv1d_1x1 without the upsampled
and the concatenated tensor (cbl_up_conv_*, csrc/up_conv.hip).
pool_bn / PoolBN: the batch norm + activation behind every local aggregation (local_aggregation_operators.py:232-238: scope 'pool_bn'), on rows that are an
input and not a product (cbl_pool_bn_*, csrc/pool_bn.hip)."""
import ctypes

import torch
from torch.autograd import Function

from . import _lib
from .local_aggregation import fan_in_init_, first_column

_i = ctypes.c_int
_f = ctypes.c_float
_ll = ctypes.c_longlong
_ACTIVATIONS = {"relu": 1, "leaky_relu": 2}              # any other string is the identity (basic_operators.py:237-241)
MAX_WIDTH = 4096


def _chk(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise TypeError(f"{name}: expected a contiguous CUDA tensor of torch.float32")
    return t


def _chk_optional(**named):
    """_chk of the arguments that are given, in their order.  Types come before every check of a shape, which is why this is not part of _bn_mode"""
    for name, t in named.items():
        if t is not None:
            _chk(t, name)


def _bn_mode(op, c_out, gamma, beta, moving_mean, moving_variance, is_training, biases=None):
    """The TF batch norm's arguments of an op (and its biases): which come together, then their lengths.  -> bn_mode (0: none, 1: batch statistics, 2: the
    moving ones), the convention of csrc/tf_bn.h"""
    if (gamma is None) != (beta is None):
        raise ValueError("{}: gamma and beta come together (both None: bn=False)".format(op))
    if gamma is None and (moving_mean is not None or moving_variance is not None):
        raise ValueError("{}: moving statistics without a batch norm".format(op))
    if (moving_mean is None) != (moving_variance is None):
        raise ValueError("{}: moving_mean and moving_variance come together".format(op))
    if gamma is not None and not is_training and moving_mean is None:
        raise ValueError("{}: is_training=False needs moving_mean and moving_variance".format(op))
    for t, name in ((biases, "biases"), (gamma, "gamma"), (beta, "beta"), (moving_mean, "moving_mean"), (moving_variance, "moving_variance")):
        if t is not None and tuple(t.shape) != (c_out,):
            raise ValueError("{}: {} of shape {}, ({},) expected".format(op, name, tuple(t.shape), c_out))
    return 0 if gamma is None else (1 if is_training else 2)


def _bn_variables(module, fdim, bn):
    """the reference's four batch-norm variables on a module (TF names): `gamma` (ones), `beta` (zeros), the buffers `moving_mean` (zeros) / `moving_variance`
    (ones); bn=False: all four None"""
    if bn:
        module.gamma = torch.nn.Parameter(torch.ones(fdim))
        module.beta = torch.nn.Parameter(torch.zeros(fdim))
        module.register_buffer("moving_mean", torch.zeros(fdim))
        module.register_buffer("moving_variance", torch.ones(fdim))
    else:
        module.gamma = module.beta = module.moving_mean = module.moving_variance = None


# What the three Functions below share.  `moving` is the tuple (moving_mean, moving_variance), which the kernels update in place under bn_mode 1: buffers, not
# inputs of the differentiated function, so they travel as one plain Python object and autograd never sees an input modified in place
def _allocator(dev):
    return lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)


def _workspace(entry, dev, *args):
    """entry: an op's cbl_*_workspace_bytes, args: its arguments"""
    return torch.empty(max(entry(*args), 1), dtype=torch.uint8, device=dev)


def _wanted(new, *specs):
    """(wanted, shape), ... -> a new tensor of that shape, or None where the gradient is not wanted"""
    return tuple(new(*shape) if wanted else None for wanted, shape in specs)


def _zeroed(*grads):
    """no rows: a gradient that is a sum over the rows is zero (nothing is launched)"""
    for g in grads:
        if g is not None:
            g.zero_()


class _Conv1d1x1(Function):
    @staticmethod
    def forward(ctx, features, weights, biases, gamma, beta, shortcut, moving, bn_mode, act, momentum, eps):
        moving_mean, moving_variance = moving
        L = _lib.lib()
        rows, c_in = features.shape
        c_out = weights.shape[1]
        new = _allocator(features.device)
        out = new(rows, c_out)
        y, save_mean, save_invstd = _wanted(new, (bn_mode, (rows, c_out)), (bn_mode, (c_out,)), (bn_mode, (c_out,)))
        ws = _workspace(L.cbl_unary_layer_workspace_bytes, features.device, _ll(rows), _i(c_in), _i(c_out)) if bn_mode == 1 else None
        _lib.check(L.cbl_unary_layer_forward(_ll(rows), _i(c_in), _i(c_out), _lib.ptr(features), _lib.ptr(weights), _lib.ptr(biases), _lib.ptr(shortcut),
                                             _i(bn_mode), _lib.ptr(gamma), _lib.ptr(beta), _f(eps), _f(momentum), _lib.ptr(moving_mean),
                                             _lib.ptr(moving_variance), _i(act), _lib.ptr(save_mean), _lib.ptr(save_invstd), _lib.ptr(y), _lib.ptr(out),
                                             _lib.ptr(ws), ctypes.c_size_t(ws.numel() if ws is not None else 0), _lib.stream_of(features)),
                   "cbl_unary_layer_forward")
        ctx.save_for_backward(features, weights, gamma, save_mean, save_invstd, y, out)
        ctx.cfg = (bn_mode, act, biases is not None, shortcut is not None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        features, weights, gamma, save_mean, save_invstd, y, out = ctx.saved_tensors
        bn_mode, act, has_bias, has_shortcut = ctx.cfg
        L = _lib.lib()
        rows, c_in = features.shape
        c_out = weights.shape[1]
        grad_out = grad_out.contiguous()
        need = ctx.needs_input_grad
        gx, gw, gb, gg, gbeta, gs = _wanted(_allocator(features.device), (need[0], (rows, c_in)), (need[1], (c_in, c_out)), (has_bias and need[2], (c_out,)),
                                            (bn_mode and need[3], (c_out,)), (bn_mode and need[4], (c_out,)), (has_shortcut and need[5], (rows, c_out)))
        if rows == 0:
            _zeroed(gw, gb, gg, gbeta)
            return (gx, gw, gb, gg, gbeta, gs) + (None,) * 5
        ws = _workspace(L.cbl_unary_layer_workspace_bytes, features.device, _ll(rows), _i(c_in), _i(c_out))
        _lib.check(L.cbl_unary_layer_backward(_ll(rows), _i(c_in), _i(c_out), _lib.ptr(features), _lib.ptr(weights), _i(bn_mode), _lib.ptr(gamma),
                                              _lib.ptr(save_mean), _lib.ptr(save_invstd), _i(act), _lib.ptr(y), _lib.ptr(out), _lib.ptr(grad_out),
                                              _lib.ptr(gx), _lib.ptr(gw), _lib.ptr(gb), _lib.ptr(gg), _lib.ptr(gbeta), _lib.ptr(gs), _lib.ptr(ws),
                                              ctypes.c_size_t(ws.numel()), _lib.stream_of(features)), "cbl_unary_layer_backward")
        return (gx, gw, gb, gg, gbeta, gs) + (None,) * 5


def conv1d_1x1(features, weights, biases=None, gamma=None, beta=None, moving_mean=None, moving_variance=None, *, is_training=True, activation_fn="relu",
               bn_momentum=0.98, bn_eps=1e-3, shortcut=None):
    """act(bn(features @ weights (+ biases)) (+ shortcut))  (rows, c_out)  (basic_operators.py:195-241).  weights: the TF variable (c_in, c_out); biases:
    with_bias; gamma / beta: the batch norm (gamma None: bn=False); moving_mean / moving_variance: updated in place when training (TF convention), used when
    not; shortcut (rows, c_out): added before the activation, which makes one call the tail of a bottleneck.  Runs on the current stream of the tensors'
    device; 1 <= c_in, c_out <= 4096."""
    _chk(features, "features"); _chk(weights, "weights")
    _chk_optional(biases=biases, gamma=gamma, beta=beta, moving_mean=moving_mean, moving_variance=moving_variance, shortcut=shortcut)
    if features.dim() != 2 or weights.dim() != 2 or features.shape[1] != weights.shape[0]:
        raise ValueError("conv1d_1x1: features {} and weights {}: (rows, c_in) and (c_in, c_out) expected".format(tuple(features.shape), tuple(weights.shape)))
    c_in, c_out = weights.shape
    if not (1 <= c_in <= MAX_WIDTH and 1 <= c_out <= MAX_WIDTH):
        raise NotImplementedError("conv1d_1x1: widths {} -> {} (1 to {} each)".format(c_in, c_out, MAX_WIDTH))
    bn_mode = _bn_mode("conv1d_1x1", c_out, gamma, beta, moving_mean, moving_variance, is_training, biases)
    if shortcut is not None and tuple(shortcut.shape) != (features.shape[0], c_out):
        raise ValueError("conv1d_1x1: shortcut of shape {}, ({}, {}) expected".format(tuple(shortcut.shape), features.shape[0], c_out))
    return _Conv1d1x1.apply(features, weights, biases, gamma, beta, shortcut, (moving_mean, moving_variance), bn_mode, _ACTIVATIONS.get(activation_fn, 0),
                            float(bn_momentum), float(bn_eps))


class Conv1d1x1(torch.nn.Module):
    """conv1d_1x1 with the reference's variables (TF names): `weights` (in_fdim, out_fdim) — init 'xavier' (glorot uniform, the default) or 'fan_in' —,
    `biases` (zeros; with_bias), and under bn `gamma` (ones), `beta` (zeros) and the buffers `moving_mean` (zeros) / `moving_variance` (ones)"""

    def __init__(self, in_fdim, out_fdim, with_bias=False, init="xavier", activation_fn="relu", bn=True, bn_momentum=0.98, bn_eps=1e-3, scope=""):
        super().__init__()
        if not (1 <= in_fdim <= MAX_WIDTH and 1 <= out_fdim <= MAX_WIDTH):
            raise NotImplementedError("Conv1d1x1: widths {} -> {} (1 to {} each)".format(in_fdim, out_fdim, MAX_WIDTH))
        if init not in ("xavier", "fan_in"):
            raise NotImplementedError("Conv1d1x1: init {} ('xavier' or 'fan_in')".format(init))
        self.activation_fn, self.bn_momentum, self.bn_eps, self.scope = activation_fn, bn_momentum, bn_eps, scope
        self.weights = torch.nn.Parameter(torch.empty(in_fdim, out_fdim))
        if init == "xavier":
            torch.nn.init.xavier_uniform_(self.weights)
        else:
            fan_in_init_(self.weights)
        self.biases = torch.nn.Parameter(torch.zeros(out_fdim)) if with_bias else None
        _bn_variables(self, out_fdim, bn)

    def tf_scopes(self):
        """variable name -> its TF variable scope (:223-235): weights / biases in the layer's own scope, the batch norm's variables under bn/"""
        bn = (self.scope + "/bn") if self.scope else "bn"
        names = {"weights": self.scope}
        if self.biases is not None:
            names["biases"] = self.scope
        if self.gamma is not None:
            names.update(gamma=bn, beta=bn, moving_mean=bn, moving_variance=bn)
        return names

    def forward(self, features, shortcut=None):
        return conv1d_1x1(features, self.weights, self.biases, self.gamma, self.beta, self.moving_mean, self.moving_variance, is_training=self.training,
                          activation_fn=self.activation_fn, bn_momentum=self.bn_momentum, bn_eps=self.bn_eps, shortcut=shortcut)


# ---------------------------------------------------------------------------------------------- the batch norm behind a local aggregation
class _PoolBN(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, moving, bn_mode, act, momentum, eps):
        moving_mean, moving_variance = moving
        L = _lib.lib()
        rows, C = x.shape
        out, save_mean, save_invstd = _wanted(_allocator(x.device), (True, (rows, C)), (bn_mode, (C,)), (bn_mode, (C,)))
        ws = _workspace(L.cbl_pool_bn_workspace_bytes, x.device, _ll(rows), _i(C)) if bn_mode == 1 else None
        _lib.check(L.cbl_pool_bn_forward(_ll(rows), _i(C), _lib.ptr(x), _i(bn_mode), _lib.ptr(gamma), _lib.ptr(beta), _f(eps), _f(momentum),
                                         _lib.ptr(moving_mean), _lib.ptr(moving_variance), _i(act), _lib.ptr(save_mean), _lib.ptr(save_invstd), _lib.ptr(out),
                                         _lib.ptr(ws), ctypes.c_size_t(ws.numel() if ws is not None else 0), _lib.stream_of(x)), "cbl_pool_bn_forward")
        ctx.save_for_backward(x, gamma, save_mean, save_invstd, out)
        ctx.cfg = (bn_mode, act)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, gamma, save_mean, save_invstd, out = ctx.saved_tensors
        bn_mode, act = ctx.cfg
        L = _lib.lib()
        rows, C = x.shape
        grad_out = grad_out.contiguous()
        need = ctx.needs_input_grad
        gx, gg, gbeta = _wanted(_allocator(x.device), (need[0], (rows, C)), (bn_mode and need[1], (C,)), (bn_mode and need[2], (C,)))
        if rows == 0:
            _zeroed(gg, gbeta)
            return (gx, gg, gbeta) + (None,) * 5
        ws = _workspace(L.cbl_pool_bn_workspace_bytes, x.device, _ll(rows), _i(C)) if bn_mode else None
        _lib.check(L.cbl_pool_bn_backward(_ll(rows), _i(C), _lib.ptr(x), _i(bn_mode), _lib.ptr(gamma), _lib.ptr(save_mean), _lib.ptr(save_invstd), _i(act),
                                          _lib.ptr(out), _lib.ptr(grad_out), _lib.ptr(gx), _lib.ptr(gg), _lib.ptr(gbeta), _lib.ptr(ws),
                                          ctypes.c_size_t(ws.numel() if ws is not None else 0), _lib.stream_of(x)), "cbl_pool_bn_backward")
        return (gx, gg, gbeta) + (None,) * 5


def pool_bn(x, gamma=None, beta=None, moving_mean=None, moving_variance=None, *, is_training=True, activation_fn="relu", bn_momentum=0.98, bn_eps=1e-3):
    """act(bn(x))  (rows, C): the batch norm and activation behind every local aggregation (local_aggregation_operators.py:232-238, :304-310, :482-488,
    :730-736; batch_norm(..., scope='pool_bn') = tf.layers.batch_normalization) — cbl_pool_bn_* (csrc/pool_bn.hip) under autograd.  gamma /
    beta: the batch norm (gamma None: bn=False, the activation alone); moving_mean / moving_variance: updated in place when training (TF convention), used
    when not.  Runs on the current stream of the tensors' device; 1 <= C <= 4096.  There is no fallback: CPU tensors raise."""
    _chk(x, "x")
    _chk_optional(gamma=gamma, beta=beta, moving_mean=moving_mean, moving_variance=moving_variance)
    if x.dim() != 2:
        raise ValueError("pool_bn: x of shape {}, (rows, C) expected".format(tuple(x.shape)))
    C = x.shape[1]
    if not 1 <= C <= MAX_WIDTH:
        raise NotImplementedError("pool_bn: width {} (1 to {})".format(C, MAX_WIDTH))
    bn_mode = _bn_mode("pool_bn", C, gamma, beta, moving_mean, moving_variance, is_training)
    return _PoolBN.apply(x, gamma, beta, (moving_mean, moving_variance), bn_mode, _ACTIVATIONS.get(activation_fn, 0), float(bn_momentum), float(bn_eps))


class PoolBN(torch.nn.Module):
    """pool_bn with the reference's variables (TF names) under its scope ('pool_bn'; PseudoGrid's is 'bn'): `gamma` (ones), `beta` (zeros) and the buffers
    `moving_mean` (zeros) / `moving_variance` (ones); bn=False: no variable at all, the activation alone"""

    def __init__(self, fdim, activation_fn="relu", bn=True, bn_momentum=0.98, bn_eps=1e-3, scope="pool_bn"):
        super().__init__()
        if not 1 <= fdim <= MAX_WIDTH:
            raise NotImplementedError("PoolBN: width {} (1 to {})".format(fdim, MAX_WIDTH))
        self.activation_fn, self.bn_momentum, self.bn_eps, self.scope = activation_fn, bn_momentum, bn_eps, scope
        _bn_variables(self, fdim, bn)

    def tf_scopes(self):
        """variable name -> its TF variable scope: all four under the layer's name (tf.layers.batch_normalization(name=scope))"""
        return {} if self.gamma is None else dict(gamma=self.scope, beta=self.scope, moving_mean=self.scope, moving_variance=self.scope)

    def forward(self, x):
        return pool_bn(x, self.gamma, self.beta, self.moving_mean, self.moving_variance, is_training=self.training, activation_fn=self.activation_fn,
                       bn_momentum=self.bn_momentum, bn_eps=self.bn_eps)


# ---------------------------------------------------------------------------------------------- the segmentation head's decoder step
class _UpConv(Function):
    @staticmethod
    def forward(ctx, coarse, inds, skip, weights, biases, gamma, beta, moving, bn_mode, act, momentum, eps):
        moving_mean, moving_variance = moving
        L = _lib.lib()
        (n1, c_up), (n2, c_skip), c_out, k = coarse.shape, skip.shape, weights.shape[1], inds.shape[1]
        new = _allocator(coarse.device)
        out = new(n2, c_out)
        y, save_mean, save_invstd = _wanted(new, (bn_mode, (n2, c_out)), (bn_mode, (c_out,)), (bn_mode, (c_out,)))
        ws = _workspace(L.cbl_up_conv_workspace_bytes, coarse.device, _ll(n2), _ll(n1), _i(c_up), _i(c_skip), _i(c_out))
        _lib.check(L.cbl_up_conv_forward(_ll(n2), _ll(n1), _i(c_up), _i(c_skip), _i(c_out), _lib.ptr(coarse), _lib.ptr(inds), _i(k), _lib.ptr(skip),
                                         _lib.ptr(weights), _lib.ptr(biases), _i(bn_mode), _lib.ptr(gamma), _lib.ptr(beta), _f(eps), _f(momentum),
                                         _lib.ptr(moving_mean), _lib.ptr(moving_variance), _i(act), _lib.ptr(save_mean), _lib.ptr(save_invstd), _lib.ptr(y),
                                         _lib.ptr(out), _lib.ptr(ws), ctypes.c_size_t(ws.numel()), _lib.stream_of(coarse)), "cbl_up_conv_forward")
        # the table's first column as the tensor the transposed table is registered under: built once per table, found again by every later backward pass
        ctx.save_for_backward(coarse, first_column(inds), skip, weights, gamma, save_mean, save_invstd, y, out)
        ctx.cfg = (bn_mode, act, biases is not None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        coarse, inds0, skip, weights, gamma, save_mean, save_invstd, y, out = ctx.saved_tensors
        bn_mode, act, has_bias = ctx.cfg
        L = _lib.lib()
        (n1, c_up), (n2, c_skip), c_out = coarse.shape, skip.shape, weights.shape[1]
        grad_out = grad_out.contiguous()
        need = ctx.needs_input_grad
        gc, gs, gw, gb, gg, gbeta = _wanted(_allocator(coarse.device), (need[0], (n1, c_up)), (need[2], (n2, c_skip)), (need[3], (c_up + c_skip, c_out)),
                                            (has_bias and need[4], (c_out,)), (bn_mode and need[5], (c_out,)), (bn_mode and need[6], (c_out,)))
        grads = (gc, None, gs, gw, gb, gg, gbeta) + (None,) * 5
        if n2 == 0:
            _zeroed(gc, gw, gb, gg, gbeta)
            return grads
        order = inv_start = inv_src = None
        if gc is not None or gw is not None:
            from . import pointops
            tr = pointops.neighbor_transpose(inds0, n1, build=True)     # shadow ids are in no segment: they receive nothing
            if tr is None:
                raise NotImplementedError("up_conv: no transposed table for {} coarse rows (cbl_neighbor_transpose's limit)".format(n1))
            order, inv_start, inv_src = tr
        ws = _workspace(L.cbl_up_conv_workspace_bytes, coarse.device, _ll(n2), _ll(n1), _i(c_up), _i(c_skip), _i(c_out))
        _lib.check(L.cbl_up_conv_backward(_ll(n2), _ll(n1), _i(c_up), _i(c_skip), _i(c_out), _lib.ptr(coarse), _lib.ptr(inds0), _i(inds0.shape[1]), _lib.ptr(skip),
                                          _lib.ptr(weights), _i(bn_mode), _lib.ptr(gamma), _lib.ptr(save_mean), _lib.ptr(save_invstd), _i(act), _lib.ptr(y),
                                          _lib.ptr(out), _lib.ptr(grad_out), _lib.ptr(order), _lib.ptr(inv_start), _lib.ptr(inv_src), _lib.ptr(gc), _lib.ptr(gs),
                                          _lib.ptr(gw), _lib.ptr(gb), _lib.ptr(gg), _lib.ptr(gbeta), _lib.ptr(ws), ctypes.c_size_t(ws.numel()),
                                          _lib.stream_of(coarse)), "cbl_up_conv_backward")
        return grads


def up_conv(coarse, upsample_inds, skip, weights, biases=None, gamma=None, beta=None, moving_mean=None, moving_variance=None, *, is_training=True,
            activation_fn="relu", bn_momentum=0.98, bn_eps=1e-3):
    """One decoder step of the segmentation head (models/heads/seg_head.py:63-67): conv1d_1x1(concat(nearest_upsample(coarse, upsample_inds), skip)) without
    the upsampled and the concatenated tensor.  coarse (n1, c_up): the coarser layer's features; upsample_inds (n2, max_num) int32, of which column 0 is
    read, an id outside [0, n1) selecting the zero row; skip (n2, c_skip): the encoder's features of the finer layer; weights: the ONE TF variable
    (c_up + c_skip, c_out) of the layer.  Everything else as conv1d_1x1 (there is no shortcut: the head has none).  1 <= c_up, c_skip, c_out;
    c_up + c_skip <= 4096, c_out <= 4096; n1 >= 1."""
    _chk(coarse, "coarse"); _chk(skip, "skip"); _chk(weights, "weights")
    if not (isinstance(upsample_inds, torch.Tensor) and upsample_inds.is_cuda and upsample_inds.dtype == torch.int32 and upsample_inds.is_contiguous()):
        raise TypeError("upsample_inds: expected a contiguous CUDA tensor of torch.int32")
    _chk_optional(biases=biases, gamma=gamma, beta=beta, moving_mean=moving_mean, moving_variance=moving_variance)
    if coarse.dim() != 2 or skip.dim() != 2 or weights.dim() != 2 or upsample_inds.dim() != 2 or upsample_inds.shape[1] < 1:
        raise ValueError("up_conv: coarse (n1, c_up), upsample_inds (n2, max_num), skip (n2, c_skip) and weights (c_up + c_skip, c_out) expected")
    (n1, c_up), (n2, c_skip), (c_in, c_out) = coarse.shape, skip.shape, weights.shape
    if upsample_inds.shape[0] != n2 or c_in != c_up + c_skip or n1 < 1:
        raise ValueError("up_conv: coarse {}, upsample_inds {}, skip {} and weights {} do not fit".format(tuple(coarse.shape), tuple(upsample_inds.shape),
                                                                                                           tuple(skip.shape), tuple(weights.shape)))
    if not (c_up >= 1 and c_skip >= 1 and c_in <= MAX_WIDTH and 1 <= c_out <= MAX_WIDTH):
        raise NotImplementedError("up_conv: widths {} + {} -> {} (each at least 1, {} at most in and out)".format(c_up, c_skip, c_out, MAX_WIDTH))
    if n2 * upsample_inds.shape[1] >= 2 ** 31:
        raise NotImplementedError("up_conv: an upsample table of {} entries (fewer than 2^31)".format(n2 * upsample_inds.shape[1]))
    bn_mode = _bn_mode("up_conv", c_out, gamma, beta, moving_mean, moving_variance, is_training, biases)
    return _UpConv.apply(coarse, upsample_inds, skip, weights, biases, gamma, beta, (moving_mean, moving_variance), bn_mode, _ACTIVATIONS.get(activation_fn, 0),
                         float(bn_momentum), float(bn_eps))


class UpConv1d1x1(Conv1d1x1):
    """up_conv with the variables, initialisers and tf_scopes() of Conv1d1x1(c_up + c_skip, out_fdim): ONE `weights` of (c_up + c_skip, out_fdim), so that a
    TF checkpoint of the layer loads unchanged"""

    def __init__(self, c_up, c_skip, out_fdim, with_bias=False, init="xavier", activation_fn="relu", bn=True, bn_momentum=0.98, bn_eps=1e-3, scope=""):
        if c_up < 1 or c_skip < 1:
            raise NotImplementedError("UpConv1d1x1: widths {} + {} (each at least 1)".format(c_up, c_skip))
        super().__init__(c_up + c_skip, out_fdim, with_bias, init, activation_fn, bn, bn_momentum, bn_eps, scope)
        self.c_up, self.c_skip = c_up, c_skip

    def forward(self, coarse, upsample_inds, skip):
        return up_conv(coarse, upsample_inds, skip, self.weights, self.biases, self.gamma, self.beta, self.moving_mean, self.moving_variance,
                       is_training=self.training, activation_fn=self.activation_fn, bn_momentum=self.bn_momentum, bn_eps=self.bn_eps)
