"""The TF side's parameter update over the library's flat-buffer entries (csrc/tf_update.hip): what the reference does between the backward
pass and the next step, which neither torch.optim.SGD nor distributed.FlatState.flat_optimizer expresses —

  * the weight loss: every `weights` variable created with a weight decay adds wd * 1/2 |w|^2 to the loss (tensorflow/models/basic_operators.py:100-130,
    :371-378, :444, local_aggregation_operators.py:720; summed by build_models.py:140-145)                                      -> weight_loss
  * tf.clip_by_norm on every variable SEPARATELY, per tower and before the towers are averaged (tensorflow/utils/average_gradients.py:21-30)   -> clip
  * tf.train.MomentumOptimizer: accum = momentum * accum + g; var -= lr * accum (tensorflow/utils/tf_graph_builder.py:99-100)               -> step

The training driver (the loop, the datasets, the configs) and the model assembly over these pieces are not part of this module.  There is no fallback: CPU
tensors raise."""
import ctypes
import re
import weakref

import numpy as np
import torch

from . import _lib

CLIP, STEP = 1, 2                                                    # CBL_TF_UPDATE_CLIP / CBL_TF_UPDATE_STEP (cbl_amd.h)


# ---------------------------------------------------------------------------------------------- which variables the reference decays
def _decay_rules():
    """module class -> does a directly held parameter of that name carry the weight loss.  One line per class of the package that holds TF-side
    parameters, each read off the reference:
      Conv1d1x1 / UpConv1d1x1   weights: _variable_with_weight_decay('weights', wd=weight_decay) basic_operators.py:225-228; biases, bn's gamma / beta: plain
                                variables (:229-235, batch_norm :134-)
      PointWiseMLP              weights, weights_l: batch_conv1d_1x1(..., weight_decay=weight_decay) local_aggregation_operators.py:591-600 -> basic_operators.py:273-276
      KPConv (pseudo_grid)      weights: _variable_with_weight_decay('weights', wd=weight_decay) local_aggregation_operators.py:720-723; the kernel points are
                                a constant (a buffer here)
      AdaptiveWeight            NOTHING: its fc layers are built with weight_decay=0 (local_aggregation_operators.py:423, :429)
      PoolBN                    nothing: gamma / beta"""
    from .convnet_blocks import _KPConvWeights
    from .local_aggregation import AdaptiveWeight, PointWiseMLP
    from .unary import Conv1d1x1, PoolBN
    weights = lambda name: name == "weights"
    return [(Conv1d1x1, weights), (_KPConvWeights, weights), (PointWiseMLP, lambda name: re.fullmatch(r"weights(_\d+)?", name) is not None),
            (AdaptiveWeight, lambda name: False), (PoolBN, lambda name: False)]


def tf_variables(*modules):
    """-> [(TF variable name, parameter, decayed)] of the modules' trainable parameters in module order: the name is the variable's tf.variable_scope nesting
    (the module's tf_scopes()) and its own name ('weights_1' of a per-pair MLP is `weights` of scope fc_1).  A module class that holds parameters and is not
    listed in _decay_rules raises: whether the reference decays a variable is read off its code, never guessed."""
    rules = _decay_rules()
    out, seen = [], set()
    for m in modules:
        if not hasattr(m, "tf_scopes"):
            raise TypeError("{}: no tf_scopes() (a module of the ConvNet side is expected)".format(type(m).__name__))
        scopes = m.tf_scopes()
        for prefix, sub in m.named_modules():
            mine = [(n, p) for n, p in sub._parameters.items() if p is not None and p.requires_grad]
            if not mine:
                continue
            rule = next((r for cls, r in rules if isinstance(sub, cls)), None)
            if rule is None:
                raise NotImplementedError("{}: a module class with parameters whose weight decay has not been read off the reference".format(type(sub).__name__))
            for n, p in mine:
                if id(p) in seen:
                    continue
                seen.add(id(p))
                key = prefix + "." + n if prefix else n
                name = "/".join(s for s in (scopes[key], re.sub(r"_\d+$", "", n)) if s)
                out.append((name, p, bool(rule(n))))
    names = [n for n, _, _ in out]
    if len(set(names)) != len(names):
        raise ValueError("TF variable names repeat ({}): give the modules distinct scopes".format(sorted({n for n in names if names.count(n) > 1})[:4]))
    return out


def decayed_variables(*modules, weight_decay):
    """-> [(TF variable name, parameter, coefficient)]: the variables the reference adds a weight loss for, in module order, each with coefficient
    `weight_decay` (config.weight_decay; s3dis: 0.001).  weight_decay <= 0: none (`if wd > 0`, basic_operators.py:127)."""
    if not weight_decay or weight_decay <= 0:
        return []
    return [(name, p, float(weight_decay)) for name, p, decayed in tf_variables(*modules) if decayed]


# ---------------------------------------------------------------------------------------------- the flat layout
class _Layout:
    """S segments of one flat buffer of `total` elements: seg_begin on the device, the chunk table of cbl_tf_update_plan, the sweeps' workspace"""

    def __init__(self, sizes, device):
        L = _lib.lib()
        self.S, self.total = len(sizes), int(sum(sizes))
        begin = np.zeros(self.S + 1, np.int64)
        begin[1:] = np.cumsum(np.asarray(sizes, np.int64))
        self.begin_host = begin
        plan = np.empty(max(1, L.cbl_tf_update_plan_bytes(self.total, self.S) // 4), np.int32)
        n_chunks = ctypes.c_longlong(0)
        _lib.check(L.cbl_tf_update_plan(self.total, self.S, begin.ctypes.data_as(ctypes.c_void_p), plan.ctypes.data_as(ctypes.c_void_p), plan.nbytes,
                                        ctypes.byref(n_chunks)), "cbl_tf_update_plan")
        self.n_chunks = n_chunks.value
        self.seg_begin = torch.from_numpy(begin).to(device)
        self.plan = torch.from_numpy(plan).to(device)
        self.ws_bytes = L.cbl_tf_update_workspace_bytes(self.total, self.S)
        self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)

    def args(self):
        return ctypes.c_longlong(self.total), ctypes.c_longlong(self.S)


def _require_cuda(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise _lib.CblError("{} must be a CUDA tensor (there is no CPU path)".format(what))
    if t.dtype != torch.float32:
        raise _lib.CblError("{} must be float32".format(what))


class _WeightLoss(torch.autograd.Function):
    """loss = sum_s wd_s / 2 |w_s|^2 over the flat parameter buffer (one call each way for the whole list); the backward pass ADDS grad_loss * wd_s * w_s into
    the flat gradient buffer, beside what the layers' backward passes accumulate into its views"""

    @staticmethod
    def forward(ctx, owner, seg_wd, decayed, *params):
        lay = owner.layout
        loss = torch.empty(1, dtype=torch.float32, device=seg_wd.device)
        seg_loss = torch.empty(lay.S, dtype=torch.float32, device=seg_wd.device)
        _lib.check(_lib.lib().cbl_tf_weight_loss_forward(*lay.args(), _lib.ptr(owner.flat_param), _lib.ptr(lay.seg_begin), _lib.ptr(seg_wd), _lib.ptr(lay.plan),
                                                         ctypes.c_longlong(lay.n_chunks), _lib.ptr(loss), _lib.ptr(seg_loss), _lib.ptr(lay.workspace),
                                                         ctypes.c_size_t(lay.ws_bytes), _lib.stream_of(loss)), "cbl_tf_weight_loss_forward")
        ctx.owner, ctx.seg_wd, ctx.decayed, ctx.n = owner, seg_wd, decayed, len(params)
        ctx.mark_non_differentiable(seg_loss)
        return loss.reshape(()), seg_loss

    @staticmethod
    def backward(ctx, grad_loss, _):
        owner, lay = ctx.owner, ctx.owner.layout
        grad_loss = grad_loss.reshape(1).to(torch.float32).contiguous()
        owner._own_grads()
        _lib.check(_lib.lib().cbl_tf_weight_loss_backward(*lay.args(), _lib.ptr(owner.flat_param), _lib.ptr(lay.seg_begin), _lib.ptr(ctx.seg_wd), _lib.ptr(lay.plan),
                                                          ctypes.c_longlong(lay.n_chunks), _lib.ptr(grad_loss), _lib.ptr(owner.flat_grad),
                                                          _lib.stream_of(grad_loss)), "cbl_tf_weight_loss_backward")
        for i in ctx.decayed:
            owner._produced[i] = True
        return (None, None, None) + (None,) * ctx.n


def weight_loss(params, coefficients, return_terms=False):
    """the reference's l2_loss (build_models.py:140-145): sum over `params` of coefficient * 1/2 |w|^2, differentiable.  The parameters must be held by ONE
    TFMomentum (their storage is its flat buffer: that is what makes this one launch each way); `coefficients` is one number per parameter or one for all.
    Parameters with coefficient 0 are not read.  return_terms: also the per-parameter terms (no gradient)."""
    params = list(params)
    if not params:
        raise ValueError("weight_loss: no parameters")
    for p in params:
        _require_cuda(p, "weight_loss: every parameter")
    coefficients = [float(coefficients)] * len(params) if not hasattr(coefficients, "__len__") else [float(c) for c in coefficients]
    if len(coefficients) != len(params):
        raise ValueError("weight_loss: {} coefficients for {} parameters".format(len(coefficients), len(params)))
    owners = {getattr(p, "_tf_momentum", None) for p in params}
    owner = owners.pop()() if len(owners) == 1 and None not in owners else None
    if owner is None:
        raise _lib.CblError("weight_loss: the parameters must be held by one TFMomentum (its flat buffer is what the kernel sweeps)")
    index = [owner._index[id(p)] for p in params]
    key = (tuple(index), tuple(coefficients))
    if key not in owner._wd_cache:
        wd = np.zeros(owner.layout.S, np.float32)
        wd[index] = coefficients
        owner._wd_cache[key] = (torch.from_numpy(wd).to(owner.flat_param.device), [i for i, c in zip(index, coefficients) if c != 0.0])
    seg_wd, decayed = owner._wd_cache[key]
    loss, seg_loss = _WeightLoss.apply(owner, seg_wd, decayed, *params)
    return (loss, seg_loss[index]) if return_terms else loss


class TFMomentum:
    """average_gradients' per-variable clip + tf.train.MomentumOptimizer over ONE flat fp32 parameter buffer, one flat gradient buffer and one flat momentum
    buffer: the parameters (and their .grad) are re-pointed as views, a variable is a segment, and the update is a norm sweep plus one apply sweep whatever the
    number of variables.

      modules_or_params   modules of the ConvNet side (names and decayed variables come from their tf_scopes(), decayed_variables) or an iterable of
                          parameters / (name, parameter) pairs (then `coefficients`, one per parameter, says which are decayed; default none)
      lr                  the learning rate, kept in DEVICE memory: set_lr(x) writes it, a captured clip_and_step() follows it
      momentum, grad_norm config.momentum (0.98), config.grad_norm (100; <= 0: no clip, as use_clip)
      weight_decay        config.weight_decay: the coefficient of every decayed variable (weight_loss() adds the loss term)
      fold_decay          add wd * w to the gradient inside the update instead of putting weight_loss() into the loss: the same step (the term's gradient is
                          exactly wd * w, and it is added before the clip either way) without the weight-loss sweeps

    Build it after the modules are on their device and before any graph capture.  A data-parallel step is clip(), all-reduce of flat_grad, step(1 / world).
    A parameter whose gradient was never produced since zero_grad() keeps its value and its momentum (tf.train.Optimizer skips a variable without a gradient;
    FlatState.step documents the same for the other side) — unless it is decayed under fold_decay, where its decay IS a gradient."""

    def __init__(self, modules_or_params, lr, momentum=0.98, grad_norm=100.0, weight_decay=0.0, fold_decay=False, coefficients=None):
        items = list(modules_or_params) if not isinstance(modules_or_params, torch.nn.Module) else [modules_or_params]
        if items and all(isinstance(m, torch.nn.Module) for m in items):
            if coefficients is not None:
                raise ValueError("TFMomentum: coefficients come from the modules' variables (decayed_variables)")
            named = [(n, p, float(weight_decay) if d and weight_decay and weight_decay > 0 else 0.0) for n, p, d in tf_variables(*items)]
        else:
            pairs = [x if isinstance(x, (tuple, list)) else ("param_%d" % i, x) for i, x in enumerate(items)]
            coefficients = [0.0] * len(pairs) if coefficients is None else [float(c) for c in coefficients]
            if len(coefficients) != len(pairs):
                raise ValueError("TFMomentum: {} coefficients for {} parameters".format(len(coefficients), len(pairs)))
            named = [(n, p, c) for (n, p), c in zip(pairs, coefficients)]
        if not named:
            raise ValueError("TFMomentum: no trainable parameters")
        if len({n for n, _, _ in named}) != len(named) or len({id(p) for _, p, _ in named}) != len(named):
            raise ValueError("TFMomentum: parameter names and parameters must be distinct")
        for n, p, _ in named:
            _require_cuda(p, "TFMomentum: parameter " + n)
        dev = named[0][1].device
        if any(p.device != dev for _, p, _ in named):
            raise _lib.CblError("TFMomentum: parameters on more than one device")
        self.names = [n for n, _, _ in named]
        self.params = [p for _, p, _ in named]
        self.coefficients = [c for _, _, c in named]
        self.momentum, self.grad_norm, self.fold_decay = float(momentum), float(grad_norm or 0.0), bool(fold_decay)
        self.layout = lay = _Layout([p.numel() for p in self.params], dev)
        self.flat_param = torch.zeros(lay.total, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(lay.total, dtype=torch.float32, device=dev)
        self.flat_accum = torch.zeros(lay.total, dtype=torch.float32, device=dev)
        self.seg_wd = torch.tensor(self.coefficients, dtype=torch.float32).to(dev)
        self.norms = torch.zeros(lay.S, dtype=torch.float32, device=dev)
        self.lr = torch.zeros(1, dtype=torch.float32, device=dev)
        self._index = {id(p): i for i, p in enumerate(self.params)}
        self._wd_cache = {}
        self.grad_views, self.accum_views = [], []
        me = weakref.ref(self)
        self._hooks = []
        with torch.no_grad():
            for i, p in enumerate(self.params):
                a, b = int(lay.begin_host[i]), int(lay.begin_host[i + 1])
                view = self.flat_param[a:b].view(p.shape)
                view.copy_(p.data)
                g = self.flat_grad[a:b].view(p.shape)
                if p.grad is not None:
                    g.copy_(p.grad)
                p.data = view                                        # the Parameter object stays (and everything that references it); its storage is the flat buffer
                p.grad = g
                p._tf_momentum = me
                self.grad_views.append(g)
                self.accum_views.append(self.flat_accum[a:b].view(p.shape))
                self._hooks.append(p.register_post_accumulate_grad_hook(self._produced_hook(i)))
        self._produced = [False] * lay.S
        self._active_host = None                                     # what seg_active holds (None: nothing uploaded yet)
        self.seg_active = torch.ones(lay.S, dtype=torch.int32, device=dev)
        self.set_lr(lr)

    def _produced_hook(self, i):
        me = weakref.ref(self)

        def hook(_param):
            owner = me()
            if owner is not None:
                owner._produced[i] = True
        return hook

    # ---- gradients
    def _own_grads(self):
        """every .grad is our view of the flat gradient buffer again: a gradient autograd put beside it (after a foreign zero_grad(set_to_none=True)) is copied
        in; a parameter without one stays idle.  Host work only (pointer comparisons) unless such a gradient is met."""
        for i, (p, g) in enumerate(zip(self.params, self.grad_views)):
            if p.grad is g:
                continue
            if p.grad is not None:
                if p.grad.data_ptr() != g.data_ptr():
                    with torch.no_grad():
                        g.copy_(p.grad)
                self._produced[i] = True
            else:
                with torch.no_grad():
                    g.zero_()
                self._produced[i] = False
            p.grad = g

    def mark_produced(self, flags=True):
        """for gradients written into flat_grad by hand (no backward pass ran): one flag for all parameters, or one per parameter"""
        self._produced = [bool(flags)] * self.layout.S if not hasattr(flags, "__len__") else [bool(f) for f in flags]
        if len(self._produced) != self.layout.S:
            raise ValueError("mark_produced: one flag per parameter")

    def zero_grad(self):
        """one fill of the flat gradient buffer; every parameter counts as without a gradient until a backward pass produces one"""
        self.flat_grad.zero_()
        for p, g in zip(self.params, self.grad_views):
            p.grad = g
        self._produced = [False] * self.layout.S

    def _sync_active(self):
        active = [bool(f or (self.fold_decay and c != 0.0)) for f, c in zip(self._produced, self.coefficients)]
        if active != self._active_host:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.CblError("TFMomentum: the set of parameters with a gradient changed under graph capture: run one eager step on the same "
                                    "backward pass before capturing")
            self.seg_active.copy_(torch.tensor(active, dtype=torch.int32))
            self._active_host = active

    # ---- the update
    def set_lr(self, lr):
        """writes the device scalar (a fill: no host synchronisation; between two replays of a captured step it changes the next replay's rate)"""
        self._lr_host = float(lr)
        self.lr.fill_(self._lr_host)

    def _update(self, mode, grad_scale):
        lay = self.layout
        self._own_grads()
        self._sync_active()
        _lib.check(_lib.lib().cbl_tf_clip_update(*lay.args(), ctypes.c_int(mode), ctypes.c_int(1 if self.fold_decay else 0), _lib.ptr(self.flat_param),
                                                 _lib.ptr(self.flat_grad), _lib.ptr(self.flat_accum), _lib.ptr(lay.seg_begin), _lib.ptr(self.seg_wd),
                                                 _lib.ptr(self.seg_active), _lib.ptr(lay.plan), ctypes.c_longlong(lay.n_chunks),
                                                 ctypes.c_float(max(self.grad_norm, 0.0)), ctypes.c_float(self.momentum), ctypes.c_float(grad_scale),
                                                 _lib.ptr(self.lr), _lib.ptr(self.norms), _lib.ptr(lay.workspace), ctypes.c_size_t(lay.ws_bytes),
                                                 _lib.stream_of(self.flat_param)), "cbl_tf_clip_update")

    def _clips(self):
        return self.grad_norm > 0 or self.fold_decay

    def clip(self):
        """every variable's gradient (with its decay under fold_decay) clipped to grad_norm, in place; -> the per-variable norms before the clip (device, (S);
        valid until the next clip).  Without a clip and without fold_decay there is nothing to do and the norms are not computed."""
        if self._clips():
            self._update(CLIP, 1.0)
        return self.norms

    def step(self, grad_scale=1.0):
        """the momentum step on the gradients as they are (clipped by clip(), averaged by the caller's all-reduce: grad_scale = 1 / world)"""
        self._update(STEP, float(grad_scale))

    def clip_and_step(self, grad_scale=1.0):
        """clip() and step() as a norm sweep plus ONE apply sweep (the gradient buffer is left holding the clipped gradients).  No allocation, no host read:
        legal under torch.cuda.graph capture"""
        self._update((CLIP | STEP) if self._clips() else STEP, float(grad_scale))

    def weight_loss(self, return_terms=False):
        """the loss term of the decayed variables (not to be added under fold_decay, which applies its gradient inside the update)"""
        return weight_loss(self.params, self.coefficients, return_terms=return_terms)

    # ---- state
    def state_dict(self):
        """the momentum by parameter name (copies), the rate and the hyper-parameters"""
        return {"momentum_buffers": {n: a.detach().clone() for n, a in zip(self.names, self.accum_views)}, "lr": self._lr_host,
                "momentum": self.momentum, "grad_norm": self.grad_norm, "fold_decay": self.fold_decay}

    def load_state_dict(self, state):
        bufs = state["momentum_buffers"]
        missing = [n for n in self.names if n not in bufs]
        extra = [n for n in bufs if n not in self._index_by_name()]
        if missing or extra:
            raise KeyError("TFMomentum.load_state_dict: missing {} / unexpected {}".format(missing[:4], extra[:4]))
        with torch.no_grad():
            for n, a in zip(self.names, self.accum_views):
                if tuple(bufs[n].shape) != tuple(a.shape):
                    raise ValueError("TFMomentum.load_state_dict: {} has shape {}, {} expected".format(n, tuple(bufs[n].shape), tuple(a.shape)))
                a.copy_(bufs[n])
        self.momentum, self.grad_norm = float(state.get("momentum", self.momentum)), float(state.get("grad_norm", self.grad_norm))
        if "lr" in state:
            self.set_lr(state["lr"])

    def _index_by_name(self):
        return {n: i for i, n in enumerate(self.names)}
