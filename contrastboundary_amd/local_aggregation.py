"""Host mirror of the TF-side local aggregation operators (value semantics of the TF1 graph code):
    kpconv (PseudoGrid)   /root/reference/tensorflow/models/local_aggregation_operators.py:620-746
    adaptive_weight       ...:316-500 (fc_num 1, 2, 3; the shipped options, config/s3dis/adapt.yaml:19-26, on kernels of their own)
    pospool               ...:15-250
    pointwise_mlp         ...:503-617 (fc_num 1, 2, 3; its batch norm and activation sit INSIDE the per-pair MLP, before the reduction: part of the kernels)
    ind_max_pool / ind_closest_pool   /root/reference/tensorflow/models/basic_operators.py:155-192
Arguments keep the reference's names and order (query_points, support_points, neighbors_indices, features, ...); the
trainable variables the TF code creates inside its variable scope (kernel weights, FC weight/bias) are explicit tensors.
The batch-norm / activation / 1x1 convs that follow in the reference are dense layers outside this path (torch)."""
import collections
import ctypes

import torch
from torch.autograd import Function

from . import _lib

_i = ctypes.c_int
_f = ctypes.c_float


def _chk(t, dtype, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise TypeError(f"{name}: expected a contiguous CUDA tensor of {dtype}")
    return t


class _KPConv(Function):
    @staticmethod
    def forward(ctx, query_points, support_points, neighbors_indices, features, kernel_points, kernel_weights, extent, influence, closest):
        n, K = neighbors_indices.shape
        n0, C = features.shape
        KP = kernel_points.shape[0]
        out = torch.empty((n, C), dtype=torch.float32, device=features.device)
        from . import pointops
        order = pointops.spatial_order(query_points)             # processing order only: same values (cbl_amd.h)
        _lib.check(_lib.lib().cbl_kpconv_forward_ordered(_i(n), _i(n0), _i(K), _i(C), _i(KP), _lib.ptr(query_points), _lib.ptr(support_points),
                                                         _lib.ptr(neighbors_indices), _lib.ptr(features), _lib.ptr(kernel_points), _lib.ptr(kernel_weights),
                                                         _f(extent), _i(influence), _i(closest), _lib.ptr(order), _lib.ptr(out),
                                                         _lib.stream_of(features)), "cbl_kpconv_forward")
        ctx.save_for_backward(query_points, support_points, neighbors_indices, features, kernel_points, kernel_weights)
        ctx.cfg = (extent, influence, closest)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, s, idx, f, kp, kw = ctx.saved_tensors
        extent, influence, closest = ctx.cfg
        n, K = idx.shape
        n0, C = f.shape
        grad_out = grad_out.contiguous()
        L = _lib.lib()
        from . import pointops
        tr = None
        if C % 4 == 0:
            # gather over the transposed neighbour table (no atomics); built where that pays, taken where it already exists
            tr = pointops.neighbor_transpose(idx, n0, build=pointops._build_table(n * K))
        if tr is not None:
            order, inv_start, inv_src = tr
            gf = torch.empty_like(f) if ctx.needs_input_grad[3] else None
            gkw = torch.empty_like(kw) if ctx.needs_input_grad[5] else None
            need = L.cbl_kpconv_backward_csr_workspace_bytes(_i(n0), _i(C), _i(kp.shape[0])) if gkw is not None else 0
            ws = torch.empty(max(need, 1), dtype=torch.uint8, device=f.device)
            rc = L.cbl_kpconv_backward_csr(_i(n), _i(n0), _i(K), _i(C), _i(kp.shape[0]), _lib.ptr(q), _lib.ptr(s), _lib.ptr(f), _lib.ptr(kp), _lib.ptr(kw),
                                           _f(extent), _i(influence), _i(closest), _lib.ptr(grad_out), _lib.ptr(order), _lib.ptr(inv_start), _lib.ptr(inv_src),
                                           _lib.ptr(gf), _lib.ptr(gkw), _lib.ptr(ws), ctypes.c_size_t(ws.numel()), _lib.stream_of(f))
            if rc != _lib.ERR_UNSUPPORTED:
                _lib.check(rc, "cbl_kpconv_backward_csr")
                return None, None, None, gf, None, gkw, None, None, None
        gf = torch.zeros_like(f) if ctx.needs_input_grad[3] else None
        gkw = torch.zeros_like(kw) if ctx.needs_input_grad[5] else None
        _lib.check(L.cbl_kpconv_backward(_i(n), _i(n0), _i(K), _i(C), _i(kp.shape[0]), _lib.ptr(q), _lib.ptr(s), _lib.ptr(idx), _lib.ptr(f),
                                         _lib.ptr(kp), _lib.ptr(kw), _f(extent), _i(influence), _i(closest), _lib.ptr(grad_out),
                                         _lib.ptr(gf), _lib.ptr(gkw), _lib.stream_of(f)), "cbl_kpconv_backward")
        return None, None, None, gf, None, gkw, None, None, None


def kpconv(query_points, support_points, neighbors_indices, features, kernel_points, kernel_weights, extent,
           KP_influence="linear", convolution_mode="sum"):
    """PseudoGrid's kernel-point convolution (depthwise): (n, C) before batch norm / activation.
    extent = KP_extent * radius / density_parameter (local_aggregation_operators.py:664)."""
    _chk(query_points, torch.float32, "query_points"); _chk(support_points, torch.float32, "support_points")
    _chk(neighbors_indices, torch.int32, "neighbors_indices"); _chk(features, torch.float32, "features")
    _chk(kernel_points, torch.float32, "kernel_points"); _chk(kernel_weights, torch.float32, "kernel_weights")
    if KP_influence not in ("linear", "constant"):
        raise NotImplementedError("KP_influence 'gaussian': radius_gaussian is not defined in the reference")
    if convolution_mode not in ("sum", "closest"):
        raise ValueError("Unknown convolution mode. Should be 'closest' or 'sum'")
    return _KPConv.apply(query_points, support_points, neighbors_indices, features, kernel_points, kernel_weights, float(extent),
                         1 if KP_influence == "linear" else 0, 1 if convolution_mode == "closest" else 0)


class _AdaptiveWeight(Function):
    @staticmethod
    def forward(ctx, query_points, support_points, neighbors_indices, features, fc_weight, fc_bias, radius, reduction_mean):
        n, K = neighbors_indices.shape
        n0, C = features.shape
        L = _lib.lib()
        pad = _padding_num(neighbors_indices, reduction_mean, _lib.stream_of(features))
        out = torch.empty((n, C), dtype=torch.float32, device=features.device)
        from . import pointops
        order = pointops.spatial_order(query_points)             # processing order only: same values (None: the rows as they are)
        _lib.check(L.cbl_adaptive_weight_forward_ordered(_i(n), _i(n0), _i(K), _i(C), _lib.ptr(query_points), _lib.ptr(support_points), _lib.ptr(neighbors_indices),
                                                         _lib.ptr(features), _f(radius), _lib.ptr(fc_weight), _lib.ptr(fc_bias), _lib.ptr(pad), _i(reduction_mean),
                                                         _lib.ptr(order), _lib.ptr(out), _lib.stream_of(features)), "cbl_adaptive_weight_forward")
        ctx.save_for_backward(query_points, support_points, neighbors_indices, features, fc_weight, fc_bias, pad)
        ctx.cfg = (radius, reduction_mean)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, s, idx, f, w, b, pad = ctx.saved_tensors
        radius, reduction_mean = ctx.cfg
        n, K = idx.shape
        n0, C = f.shape
        grad_out = grad_out.contiguous()
        L = _lib.lib()
        need_f, need_w, need_b = ctx.needs_input_grad[3], ctx.needs_input_grad[4], ctx.needs_input_grad[5]
        from . import pointops
        tr = None
        if C % 4 == 0:
            # gather over the transposed neighbour table (no atomics, deterministic); built where that pays, taken where it already exists
            tr = pointops.neighbor_transpose(idx, n0, build=pointops._build_table(n * K))
        if tr is not None:
            order, inv_start, inv_src = tr
            gf = torch.empty_like(f) if need_f else None
            gw = torch.empty_like(w) if need_w else None
            gb = torch.empty_like(b) if need_b else None
            ws = torch.empty(L.cbl_adaptive_weight_backward_csr_workspace_bytes(_i(n), _i(n0), _i(C)), dtype=torch.uint8, device=f.device)
            rc = L.cbl_adaptive_weight_backward_csr(_i(n), _i(n0), _i(K), _i(C), _lib.ptr(q), _lib.ptr(s), _lib.ptr(idx), _lib.ptr(f), _f(radius), _lib.ptr(w),
                                                    _lib.ptr(b), _lib.ptr(pad), _i(reduction_mean), _lib.ptr(grad_out), _lib.ptr(order), _lib.ptr(inv_start),
                                                    _lib.ptr(inv_src), _lib.ptr(gf), _lib.ptr(gw), _lib.ptr(gb), _lib.ptr(ws), ctypes.c_size_t(ws.numel()),
                                                    _lib.stream_of(f))
            if rc != _lib.ERR_UNSUPPORTED:
                _lib.check(rc, "cbl_adaptive_weight_backward_csr")
                return None, None, None, gf, gw, gb, None, None
        gf = torch.zeros_like(f) if need_f else None
        gw = torch.zeros_like(w) if need_w else None
        gb = torch.zeros_like(b) if need_b else None
        _lib.check(L.cbl_adaptive_weight_backward(_i(n), _i(n0), _i(K), _i(C), _lib.ptr(q), _lib.ptr(s), _lib.ptr(idx), _lib.ptr(f), _f(radius),
                                                  _lib.ptr(w), _lib.ptr(b), _lib.ptr(pad), _i(reduction_mean), _lib.ptr(grad_out),
                                                  _lib.ptr(gf), _lib.ptr(gw), _lib.ptr(gb), _lib.stream_of(f)), "cbl_adaptive_weight_backward")
        return None, None, None, gf, gw, gb, None, None


ADAPTIVE_WEIGHT_INPUTS = ("dp", "df", "dp_df", "fj", "dp_fj", "fi_df", "dp_fi_df")
_AW_SOFTMAX = {None: 0, False: 0, "dense": 1, "sparse": 1, "mask": 1, "unmask": 2}
_AW_REDUCTIONS = {"sum": 0, "mean": 1, "avg": 1, "max": 2}
_NO_TABLE = "{}: no transposed neighbour table for more than 2^20 support points, and there is no scatter form"


def _padding_num(idx, red_is_mean, stream):
    """-> the one-int device tensor behind 'mean' (max(idx), :466-470): filled only when the reduction is 'mean'"""
    pad = torch.empty(1, dtype=torch.int32, device=idx.device)
    if red_is_mean:
        _lib.check(_lib.lib().cbl_index_max(ctypes.c_longlong(idx.numel()), _lib.ptr(idx), _lib.ptr(pad), stream), "cbl_index_max")
    return pad


def _pair_table(idx, n0, op_name):
    """-> (order, inv_start, inv_src) of the transposed neighbour table, built if need be; the operators without a scatter form refuse where there is none"""
    from . import pointops
    tr = pointops.neighbor_transpose(idx, n0, build=True)
    if tr is None:
        raise NotImplementedError(_NO_TABLE.format(op_name))
    return tr


def _center_rows_to_support(gc, idx, n0, width, op_name):
    """per-query rows (n, width) onto the centre rows they came from (shadow_features[idx[:, 0]]) -> (n0, width): the row scatter as a gather over the table
    of that one column"""
    tr0 = _pair_table(idx[:, :1].contiguous(), n0, op_name)
    gcen = torch.empty((n0, width), dtype=torch.float32, device=gc.device)
    _lib.check(_lib.lib().cbl_grouping_backward_csr_rows(_i(n0), _i(width), _i(width), _i(0), _lib.ptr(gc), _lib.ptr(tr0[0]), _lib.ptr(tr0[1]), _lib.ptr(tr0[2]),
                                                         _lib.ptr(gcen), _lib.stream_of(gc)), "cbl_grouping_backward_csr_rows")
    return gcen


def _aw_d_in(local_input_feature, in_fdim):
    blocks = local_input_feature.split("_")
    return 3 * ("dp" in blocks) + in_fdim * sum(b in blocks for b in ("fi", "df", "fj"))


def _aw_options(local_input_feature, shared_channels, weight_softmax, reduction, in_fdim):
    """-> S = min(shared_channels, in_fdim); refuses what the kernels (and for 'rscnn' / 'gac' this mirror) do not cover, naming the option"""
    if local_input_feature not in ADAPTIVE_WEIGHT_INPUTS:
        raise NotImplementedError("local_input_feature {} not supported in AdaptiveWeight (one of {})".format(local_input_feature, ", ".join(ADAPTIVE_WEIGHT_INPUTS)))
    if weight_softmax not in _AW_SOFTMAX:
        raise NotImplementedError("weight_softmax {!r} not supported in AdaptiveWeight (False, 'dense', 'sparse', 'mask' or 'unmask')".format(weight_softmax))
    if reduction not in _AW_REDUCTIONS:
        raise NotImplementedError("Reduction {} not supported in AdaptiveWeight".format(reduction))
    S = min(int(shared_channels), in_fdim)
    if S < 1 or in_fdim % S != 0:
        raise NotImplementedError("shared_channels {}: {} features do not divide into groups of it (the reference's reshape fails as well)".format(shared_channels, in_fdim))
    if S not in (1, 2, 4) and S % 4 != 0:
        raise NotImplementedError("shared_channels {}: 1, 2, 4 or a multiple of 4".format(shared_channels))
    return S


class _AdaptiveWeightGeneral(Function):
    """the two entries of csrc/adaptive_weight_general.hip around the folded per-point terms (cbl_amd.h, a14 AdaptiveWeight, every option)"""

    @staticmethod
    def forward(ctx, query_points, support_points, neighbors_indices, features, center_term, neighbor_term, w_pos, bias, radius, softmax, red):
        n, K = neighbors_indices.shape
        n0, C = features.shape
        M = bias.shape[0]
        L = _lib.lib()
        dev = features.device
        st = _lib.stream_of(features)
        pad = _padding_num(neighbors_indices, red == 1, st)
        out = torch.empty((n, C), dtype=torch.float32, device=dev)
        _lib.check(L.cbl_adaptive_weight_general_forward(_i(n), _i(n0), _i(K), _i(C), _i(M), _lib.ptr(query_points), _lib.ptr(support_points),
                                                         _lib.ptr(neighbors_indices), _lib.ptr(features), _lib.ptr(center_term), _lib.ptr(neighbor_term),
                                                         _lib.ptr(w_pos), _lib.ptr(bias), _f(radius), _i(softmax), _i(red), _lib.ptr(pad), _lib.ptr(out),
                                                         None, ctypes.c_size_t(0), st), "cbl_adaptive_weight_general_forward")
        ctx.save_for_backward(query_points, support_points, neighbors_indices, features, center_term, neighbor_term, w_pos, bias, pad, out)
        ctx.cfg = (radius, softmax, red)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, s, idx, f, cen, nbr, wp, bias, pad, out = ctx.saved_tensors
        radius, softmax, red = ctx.cfg
        n, K = idx.shape
        n0, C = f.shape
        M = bias.shape[0]
        grad_out = grad_out.contiguous()
        L = _lib.lib()
        dev = f.device
        st = _lib.stream_of(f)
        need = ctx.needs_input_grad
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        gf = new(n0, C) if need[3] else None
        gc = new(n, M) if cen is not None and need[4] else None
        gn = new(n0, M) if nbr is not None and need[5] else None
        gwp = new(3, M) if wp is not None and need[6] else None
        gb = new(M) if need[7] else None
        order = inv_start = inv_src = None
        if gf is not None or gn is not None:
            order, inv_start, inv_src = _pair_table(idx, n0, "adaptive_weight")
        ws = torch.empty(max(L.cbl_adaptive_weight_general_workspace_bytes(_i(n), _i(n0), _i(K), _i(C), _i(M)), 1), dtype=torch.uint8, device=dev)
        _lib.check(L.cbl_adaptive_weight_general_backward_csr(_i(n), _i(n0), _i(K), _i(C), _i(M), _lib.ptr(q), _lib.ptr(s), _lib.ptr(idx), _lib.ptr(f),
                                                              _lib.ptr(cen), _lib.ptr(nbr), _lib.ptr(wp), _lib.ptr(bias), _f(radius), _i(softmax), _i(red),
                                                              _lib.ptr(pad), _lib.ptr(out), _lib.ptr(grad_out), _lib.ptr(order), _lib.ptr(inv_start),
                                                              _lib.ptr(inv_src), _lib.ptr(gf), _lib.ptr(gc), _lib.ptr(gn), _lib.ptr(gwp), _lib.ptr(gb),
                                                              _lib.ptr(ws), ctypes.c_size_t(ws.numel()), st), "cbl_adaptive_weight_general_backward_csr")
        gcen = _center_rows_to_support(gc, idx, n0, M, "adaptive_weight") if gc is not None else None
        return None, None, None, gf, gcen, gn, gwp, gb, None, None, None


class _AdaptiveWeightMLP(Function):
    """the two entries of csrc/adaptive_weight_mlp.hip around the folded per-point terms (cbl_amd.h, a14 AdaptiveWeight with fc_num 2 and 3);
    hidden_w (layers, M, M) / hidden_b (layers, M): the layers behind the first, stacked"""

    @staticmethod
    def forward(ctx, query_points, support_points, neighbors_indices, features, center_term, neighbor_term, w_pos, bias, hidden_w, hidden_b, radius, softmax,
                red, act):
        n, K = neighbors_indices.shape
        n0, C = features.shape
        M, layers = bias.shape[0], hidden_w.shape[0]
        L = _lib.lib()
        dev = features.device
        st = _lib.stream_of(features)
        pad = _padding_num(neighbors_indices, red == 1, st)
        out = torch.empty((n, C), dtype=torch.float32, device=dev)
        _lib.check(L.cbl_adaptive_weight_mlp_forward(_i(n), _i(n0), _i(K), _i(C), _i(M), _lib.ptr(query_points), _lib.ptr(support_points),
                                                     _lib.ptr(neighbors_indices), _lib.ptr(features), _lib.ptr(center_term), _lib.ptr(neighbor_term),
                                                     _lib.ptr(w_pos), _lib.ptr(bias), _i(layers), _lib.ptr(hidden_w), _lib.ptr(hidden_b), _i(act), _f(radius),
                                                     _i(softmax), _i(red), _lib.ptr(pad), _lib.ptr(out), None, ctypes.c_size_t(0), st),
                   "cbl_adaptive_weight_mlp_forward")
        ctx.save_for_backward(query_points, support_points, neighbors_indices, features, center_term, neighbor_term, w_pos, bias, hidden_w, hidden_b, pad, out)
        ctx.cfg = (radius, softmax, red, act)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, s, idx, f, cen, nbr, wp, bias, hw, hb, pad, out = ctx.saved_tensors
        radius, softmax, red, act = ctx.cfg
        n, K = idx.shape
        n0, C = f.shape
        M, layers = bias.shape[0], hw.shape[0]
        grad_out = grad_out.contiguous()
        L = _lib.lib()
        dev = f.device
        st = _lib.stream_of(f)
        need = ctx.needs_input_grad
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        gf = new(n0, C) if need[3] else None
        gc = new(n, M) if cen is not None and need[4] else None
        gn = new(n0, M) if nbr is not None and need[5] else None
        gwp = new(3, M) if wp is not None and need[6] else None
        gb = new(M) if need[7] else None
        ghw = new(layers, M, M) if need[8] else None
        ghb = new(layers, M) if need[9] else None
        order = inv_start = inv_src = None
        if gf is not None or gn is not None:
            order, inv_start, inv_src = _pair_table(idx, n0, "adaptive_weight")
        ws = torch.empty(max(L.cbl_adaptive_weight_mlp_workspace_bytes(_i(n), _i(n0), _i(K), _i(C), _i(M), _i(layers)), 1), dtype=torch.uint8, device=dev)
        _lib.check(L.cbl_adaptive_weight_mlp_backward_csr(_i(n), _i(n0), _i(K), _i(C), _i(M), _lib.ptr(q), _lib.ptr(s), _lib.ptr(idx), _lib.ptr(f),
                                                          _lib.ptr(cen), _lib.ptr(nbr), _lib.ptr(wp), _lib.ptr(bias), _i(layers), _lib.ptr(hw), _lib.ptr(hb),
                                                          _i(act), _f(radius), _i(softmax), _i(red), _lib.ptr(pad), _lib.ptr(out), _lib.ptr(grad_out),
                                                          _lib.ptr(order), _lib.ptr(inv_start), _lib.ptr(inv_src), _lib.ptr(gf), _lib.ptr(gc), _lib.ptr(gn),
                                                          _lib.ptr(gwp), _lib.ptr(gb), _lib.ptr(ghw), _lib.ptr(ghb), _lib.ptr(ws),
                                                          ctypes.c_size_t(ws.numel()), st), "cbl_adaptive_weight_mlp_backward_csr")
        gcen = _center_rows_to_support(gc, idx, n0, M, "adaptive_weight") if gc is not None else None
        return None, None, None, gf, gcen, gn, gwp, gb, ghw, ghb, None, None, None, None


_AW_MLP_M = (16, 144)          # the widths csrc/adaptive_weight_mlp.hip takes (one matrix tile .. the ConvNet's stage-2 width)


def _aw_mlp_limits(fc_num, M, K=None):
    """refuses the depths and widths the per-pair MLP kernels do not cover, naming fc_num"""
    if fc_num > 3:
        raise NotImplementedError("adaptive_weight.fc_num {}: fc_num 1, 2 and 3 are implemented".format(fc_num))
    if not _AW_MLP_M[0] <= M <= _AW_MLP_M[1]:
        raise NotImplementedError("adaptive_weight.fc_num {}: only fc_num 1 is implemented for {} weight groups (the per-pair MLP kernels take {} to {})".format(
            fc_num, M, *_AW_MLP_M))
    if K is not None and (K > 128 or (K > 48 and M > 64)):
        raise NotImplementedError("adaptive_weight.fc_num {}: {} neighbours with {} weight groups (at most 48, or 128 up to 64 groups)".format(fc_num, K, M))


def adaptive_weight(query_points, support_points, neighbors_indices, features, radius, fc_weight, fc_bias, reduction="mean", *,
                    local_input_feature="dp", shared_channels=1, weight_softmax=False, fc_hidden=(), activation_fn="relu"):
    """AdaptiveWeight aggregation_feature (n, C) before batch norm / activation / output_conv (tensorflow/models/local_aggregation_operators.py:316-480;
    options as config.adaptive_weight.*) with fc_num 1 + len(fc_hidden) (1, 2 or 3).  fc_weight: the TF variable fc_1/weights (D_in, M), M = C / min(shared_channels, C), rows in the
    concatenation order of :386-401; fc_bias (M).
    The shipped options ('dp', shared_channels 1, no softmax, sum / mean) run the kernels specialised for them.  Everything else: one FC layer is linear in
    the concatenated blocks, y = dp @ W_p + (f @ (W_fi - W_df))[idx[:, 0]] + (f @ (W_df + W_fj))[idx] + bias — the two per-point products are dense layers
    here (autograd carries the fold and the weight gradient), the per-pair part is csrc/adaptive_weight_general.hip.
    weight_softmax 'dense' / 'sparse' / 'mask' are one masked softmax over the real neighbours; for a query without any real neighbour it gives zero
    weights (so do the reference's 'sparse' and, in effect, 'dense'; its 'mask' divides 0 by 0 there and yields NaN — such a query does not occur in its
    pipelines, where column 0 is the point itself).
    fc_hidden: (weight (M, M), bias (M)) of every layer behind the first, in order (:419-430; TF's (in, out) weights).  The first layer is followed by
    activation_fn ('relu', 'leaky_relu' with alpha 0.2, anything else the identity: basic_operators.py:285-289), so are the layers between; the last has
    none.  The first layer keeps its fold and its dense products; the per-pair MLP is csrc/adaptive_weight_mlp.hip (16 <= M <= 144; K <= 48, or <= 128 up
    to M = 64).  With fc_hidden empty, activation_fn is unused and the call is fc_num 1's."""
    S = _aw_options(local_input_feature, shared_channels, weight_softmax, reduction, features.shape[1])
    C = features.shape[1]
    M = C // S
    if tuple(fc_weight.shape) != (_aw_d_in(local_input_feature, C), M):
        raise ValueError("fc_weight: shape {}, local_input_feature {} of {} features with shared_channels {} has ({}, {})".format(
            tuple(fc_weight.shape), local_input_feature, C, shared_channels, _aw_d_in(local_input_feature, C), M))
    _chk(query_points, torch.float32, "query_points"); _chk(support_points, torch.float32, "support_points")
    _chk(neighbors_indices, torch.int32, "neighbors_indices"); _chk(features, torch.float32, "features")
    _chk(fc_weight, torch.float32, "fc_weight"); _chk(fc_bias, torch.float32, "fc_bias")
    softmax, red = _AW_SOFTMAX[weight_softmax], _AW_REDUCTIONS[reduction]
    fc_hidden = tuple(fc_hidden)
    if fc_hidden:
        _aw_mlp_limits(1 + len(fc_hidden), M, neighbors_indices.shape[1])
        for l, (w, b) in enumerate(fc_hidden, 1):
            _chk(w, torch.float32, "fc_hidden[{}] weight".format(l - 1)); _chk(b, torch.float32, "fc_hidden[{}] bias".format(l - 1))
            if tuple(w.shape) != (M, M) or tuple(b.shape) != (M,):
                raise ValueError("fc_hidden[{}]: shapes {} and {}, a layer of {} weight groups has ({}, {}) and ({},)".format(
                    l - 1, tuple(w.shape), tuple(b.shape), M, M, M, M))
    if not fc_hidden and local_input_feature == "dp" and S == 1 and softmax == 0 and red != 2:
        return _AdaptiveWeight.apply(query_points, support_points, neighbors_indices, features, fc_weight, fc_bias, float(radius), red)
    if C % 4 != 0 or C > 1152:
        raise NotImplementedError("adaptive_weight: {} features (a multiple of 4 up to 1152)".format(C))
    if neighbors_indices.shape[1] > 128:
        raise NotImplementedError("adaptive_weight: {} neighbours (at most 128)".format(neighbors_indices.shape[1]))
    from . import dense
    blocks, o = {}, 0
    for name in local_input_feature.split("_"):
        rows = 3 if name == "dp" else C
        blocks[name] = fc_weight[o:o + rows]
        o += rows
    w_pos = blocks["dp"].contiguous() if "dp" in blocks else None
    center_term = neighbor_term = None
    if "fi" in blocks or "df" in blocks:
        w_c = blocks["fi"] - blocks["df"] if "fi" in blocks else -blocks["df"]
        center_term = dense.linear(features, w_c.t()).contiguous()
    if "df" in blocks or "fj" in blocks:
        w_n = blocks["df"] if "df" in blocks else blocks["fj"]              # (no mode of :386-401 has both)
        neighbor_term = dense.linear(features, w_n.t()).contiguous()
    if fc_hidden:
        return _AdaptiveWeightMLP.apply(query_points, support_points, neighbors_indices, features, center_term, neighbor_term, w_pos, fc_bias,
                                        torch.stack([w for w, _ in fc_hidden]), torch.stack([b for _, b in fc_hidden]), float(radius), softmax, red,
                                        _PW_ACTIVATIONS.get(activation_fn, 0))
    return _AdaptiveWeightGeneral.apply(query_points, support_points, neighbors_indices, features, center_term, neighbor_term, w_pos, fc_bias, float(radius),
                                        softmax, red)


def fan_in_init_(weights):
    """tf.contrib.layers.variance_scaling_initializer(factor=1.0, mode='FAN_IN', uniform=False): a normal of standard deviation sqrt(1.3 / fan_in)
    truncated at two standard deviations; fan_in = the rows of a TF (in, out) weight"""
    std = (1.3 / weights.shape[0]) ** 0.5
    with torch.no_grad():
        return torch.nn.init.trunc_normal_(weights, 0.0, std, -2 * std, 2 * std)


class AdaptiveWeight(torch.nn.Module):
    """the operator with its variables, drawn as the reference's 'fan_in' initializer does (basic_operators.py:120-121) with zero biases: `weights` (D_in, M) /
    `biases` of the first layer, and for fc_num 2 and 3 `weights_1`, `biases_1` (, `weights_2`, `biases_2`) (M, M) / (M) of the layers behind it (:419-430)"""

    def __init__(self, in_fdim, local_input_feature="dp", shared_channels=1, fc_num=1, weight_softmax=False, reduction="mean", activation_fn="relu"):
        super().__init__()
        if fc_num < 1:
            raise ValueError("adaptive_weight.fc_num {}: at least 1".format(fc_num))
        S = _aw_options(local_input_feature, shared_channels, weight_softmax, reduction, in_fdim)
        d_in, M = _aw_d_in(local_input_feature, in_fdim), in_fdim // S
        if fc_num != 1:
            _aw_mlp_limits(fc_num, M)
        self.local_input_feature, self.shared_channels, self.fc_num = local_input_feature, shared_channels, fc_num
        self.weight_softmax, self.reduction, self.activation_fn = weight_softmax, reduction, activation_fn
        self.weights = torch.nn.Parameter(torch.empty(d_in, M))
        fan_in_init_(self.weights)
        self.biases = torch.nn.Parameter(torch.zeros(M))
        for l in range(1, fc_num):
            w = torch.nn.Parameter(torch.empty(M, M))
            fan_in_init_(w)
            setattr(self, "weights_{}".format(l), w)
            setattr(self, "biases_{}".format(l), torch.nn.Parameter(torch.zeros(M)))

    def tf_scopes(self):
        """parameter name -> the TF variable scope of its layer (:419-430): fc_0 .. fc_{fc_num-2} for the layers with an activation, fc_{fc_num} for the
        last one — the number fc_num - 1 is skipped, which someone loading a reference checkpoint has to know"""
        scope = lambda l: "fc_{}".format(l if l < self.fc_num - 1 else self.fc_num)
        names = {"weights": scope(0), "biases": scope(0)}
        for l in range(1, self.fc_num):
            names["weights_{}".format(l)] = names["biases_{}".format(l)] = scope(l)
        return names

    def forward(self, query_points, support_points, neighbors_indices, features, radius):
        hidden = [(getattr(self, "weights_{}".format(l)), getattr(self, "biases_{}".format(l))) for l in range(1, self.fc_num)]
        return adaptive_weight(query_points, support_points, neighbors_indices, features, radius, self.weights, self.biases, self.reduction,
                               local_input_feature=self.local_input_feature, shared_channels=self.shared_channels, weight_softmax=self.weight_softmax,
                               fc_hidden=hidden, activation_fn=self.activation_fn)


POSPOOL_EMBEDDINGS = {"one": 0, "xyz": 1, "distance": 2, "exp_-d": 3, "direction_exp_-d": 4, "direction_d": 5, "sin_cos": 6,
                      "two_order": 7, "three_order": 8}
_POSPOOL_REDUCTIONS = {"sum": 0, "mean": 1, "avg": 1, "max": 2}


class _PosPool(Function):
    @staticmethod
    def forward(ctx, query_points, support_points, neighbors_indices, features, radius, pe, red):
        n, K = neighbors_indices.shape
        n0, C = features.shape
        L = _lib.lib()
        pad = _padding_num(neighbors_indices, red == 1, _lib.stream_of(features))
        out = torch.empty((n, C), dtype=torch.float32, device=features.device)
        _lib.check(L.cbl_pospool_forward(_i(n), _i(n0), _i(K), _i(C), _lib.ptr(query_points), _lib.ptr(support_points), _lib.ptr(neighbors_indices),
                                         _lib.ptr(features), _f(radius), _i(pe), _i(red), _lib.ptr(pad), _lib.ptr(out), _lib.stream_of(features)),
                   "cbl_pospool_forward")
        ctx.save_for_backward(query_points, support_points, neighbors_indices, features, pad)
        ctx.cfg = (radius, pe, red)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, s, idx, f, pad = ctx.saved_tensors
        radius, pe, red = ctx.cfg
        n, K = idx.shape
        n0, C = f.shape
        grad_out = grad_out.contiguous()
        L = _lib.lib()
        if red != 2 and C % 4 == 0:
            # 'sum' / 'mean': a gather over the transposed neighbour table (no atomics, deterministic), built where that pays, taken where it exists
            from . import pointops
            tr = pointops.neighbor_transpose(idx, n0, build=pointops._build_table(n * K))
            if tr is not None:
                order, inv_start, inv_src = tr
                gf = torch.empty_like(f)
                ws = torch.empty(L.cbl_pospool_backward_csr_workspace_bytes(_i(n)), dtype=torch.uint8, device=f.device)
                rc = L.cbl_pospool_backward_csr(_i(n), _i(n0), _i(K), _i(C), _lib.ptr(q), _lib.ptr(s), _lib.ptr(idx), _f(radius), _i(pe), _i(red), _lib.ptr(pad),
                                                _lib.ptr(grad_out), _lib.ptr(order), _lib.ptr(inv_start), _lib.ptr(inv_src), _lib.ptr(gf), _lib.ptr(ws),
                                                ctypes.c_size_t(ws.numel()), _lib.stream_of(f))
                if rc != _lib.ERR_UNSUPPORTED:
                    _lib.check(rc, "cbl_pospool_backward_csr")
                    return None, None, None, gf, None, None, None
        gf = torch.zeros_like(f)
        _lib.check(_lib.lib().cbl_pospool_backward(_i(n), _i(n0), _i(K), _i(C), _lib.ptr(q), _lib.ptr(s), _lib.ptr(idx), _lib.ptr(f), _f(radius),
                                                   _i(pe), _i(red), _lib.ptr(pad), _lib.ptr(grad_out), _lib.ptr(gf), _lib.stream_of(f)),
                   "cbl_pospool_backward")
        return None, None, None, gf, None, None, None


def pospool(query_points, support_points, neighbors_indices, features, radius, position_embedding="sin_cos", reduction="mean"):
    """PosPool aggregation_feature (n, C) before pool_bn / activation / output_conv
    (tensorflow/models/local_aggregation_operators.py:15-250; options as config.pospool.position_embedding / .reduction)."""
    _chk(query_points, torch.float32, "query_points"); _chk(support_points, torch.float32, "support_points")
    _chk(neighbors_indices, torch.int32, "neighbors_indices"); _chk(features, torch.float32, "features")
    if position_embedding not in POSPOOL_EMBEDDINGS:
        raise NotImplementedError("position_embedding [{}] not supported in PosPool ".format(position_embedding))
    if reduction not in _POSPOOL_REDUCTIONS:
        raise NotImplementedError("Reduction {} not supported in PosPool".format(reduction))
    return _PosPool.apply(query_points, support_points, neighbors_indices, features, float(radius), POSPOOL_EMBEDDINGS[position_embedding],
                          _POSPOOL_REDUCTIONS[reduction])


POINTWISE_MLP_INPUTS = ("dp_fj", "fi_df", "dp_fi_df", "dp_fi_df_fj")
_PW_REDUCTIONS = {"sum": 0, "mean": 1, "max": 2}
_PW_ACTIVATIONS = {"relu": 1, "leaky_relu": 2}          # any other string is the identity (basic_operators.py:285-289)


class _PointWiseMLP(Function):
    """the two entries of csrc/pointwise_mlp.hip around the folded per-point terms (cbl_amd.h, a14 PointWiseMLP)"""

    @staticmethod
    def forward(ctx, query_points, support_points, neighbors_indices, center_term, neighbor_term, w_pos, gamma, beta, moving_mean, moving_variance,
                radius, bn_mode, act, red, momentum, eps):
        n, K = neighbors_indices.shape
        n0, C = neighbor_term.shape
        L = _lib.lib()
        dev = neighbor_term.device
        st = _lib.stream_of(neighbor_term)
        pad = _padding_num(neighbors_indices, red == 1, st)
        out = torch.empty((n, C), dtype=torch.float32, device=dev)
        save_mean = torch.empty(C, dtype=torch.float32, device=dev) if bn_mode else None
        save_invstd = torch.empty(C, dtype=torch.float32, device=dev) if bn_mode else None
        ws = torch.empty(max(L.cbl_pointwise_mlp_workspace_bytes(_i(n), _i(n0), _i(K), _i(C)), 1), dtype=torch.uint8, device=dev)
        _lib.check(L.cbl_pointwise_mlp_forward(_i(n), _i(n0), _i(K), _i(C), _lib.ptr(query_points), _lib.ptr(support_points), _lib.ptr(neighbors_indices),
                                               _lib.ptr(center_term), _lib.ptr(neighbor_term), _lib.ptr(w_pos), _f(radius), _i(bn_mode), _lib.ptr(gamma),
                                               _lib.ptr(beta), _f(eps), _f(momentum), _lib.ptr(moving_mean), _lib.ptr(moving_variance), _i(act), _i(red),
                                               _lib.ptr(pad), _lib.ptr(save_mean), _lib.ptr(save_invstd), _lib.ptr(out), _lib.ptr(ws),
                                               ctypes.c_size_t(ws.numel()), st), "cbl_pointwise_mlp_forward")
        ctx.save_for_backward(query_points, support_points, neighbors_indices, center_term, neighbor_term, w_pos, gamma, beta, save_mean, save_invstd, pad, out)
        ctx.cfg = (radius, bn_mode, act, red)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, s, idx, cen, nbr, wp, gamma, beta, save_mean, save_invstd, pad, out = ctx.saved_tensors
        radius, bn_mode, act, red = ctx.cfg
        n, K = idx.shape
        n0, C = nbr.shape
        grad_out = grad_out.contiguous()
        L = _lib.lib()
        dev = nbr.device
        st = _lib.stream_of(nbr)
        need = ctx.needs_input_grad
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        gc = new(n, C) if cen is not None and need[3] else None
        gn = new(n0, C) if need[4] else None
        gwp = new(3, C) if wp is not None and need[5] else None
        gg = new(C) if gamma is not None and need[6] else None
        gb = new(C) if beta is not None and need[7] else None
        order = inv_start = inv_src = None
        if gn is not None:
            order, inv_start, inv_src = _pair_table(idx, n0, "pointwise_mlp")
        ws = torch.empty(max(L.cbl_pointwise_mlp_workspace_bytes(_i(n), _i(n0), _i(K), _i(C)), 1), dtype=torch.uint8, device=dev)
        _lib.check(L.cbl_pointwise_mlp_backward_csr(_i(n), _i(n0), _i(K), _i(C), _lib.ptr(q), _lib.ptr(s), _lib.ptr(idx), _lib.ptr(cen), _lib.ptr(nbr),
                                                    _lib.ptr(wp), _f(radius), _i(bn_mode), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(save_mean),
                                                    _lib.ptr(save_invstd), _i(act), _i(red), _lib.ptr(pad), _lib.ptr(out), _lib.ptr(grad_out),
                                                    _lib.ptr(order), _lib.ptr(inv_start), _lib.ptr(inv_src), _lib.ptr(gc), _lib.ptr(gn), _lib.ptr(gwp),
                                                    _lib.ptr(gg), _lib.ptr(gb), _lib.ptr(ws), ctypes.c_size_t(ws.numel()), st), "cbl_pointwise_mlp_backward_csr")
        gcen = _center_rows_to_support(gc, idx, n0, C, "pointwise_mlp") if gc is not None else None
        return (None, None, None, gcen, gn, gwp, gg, gb) + (None,) * 8


class _PointWiseMLPLayers(Function):
    """the two entries of csrc/pointwise_mlp_layers.hip around the folded per-point terms of fc_0 (cbl_amd.h, a14 PointWiseMLP with fc_num 2 and 3).
    hidden_w: the weights behind the first layer, flattened and packed in order; gamma / beta / moving_mean / moving_variance: packed over the layers
    (layers * H + C_out), the moving statistics as ONE buffer the kernels update in place (the caller copies it back)"""

    @staticmethod
    def forward(ctx, query_points, support_points, neighbors_indices, center_term, neighbor_term, w_pos, hidden_w, gamma, beta, moving_mean, moving_variance,
                radius, bn_mode, act, red, momentum, eps, C_out, layers):
        n, K = neighbors_indices.shape
        n0, H = neighbor_term.shape
        L = _lib.lib()
        dev = neighbor_term.device
        st = _lib.stream_of(neighbor_term)
        pad = _padding_num(neighbors_indices, red == 1, st)
        out = torch.empty((n, C_out), dtype=torch.float32, device=dev)
        WT = layers * H + C_out
        save_mean = torch.empty(WT, dtype=torch.float32, device=dev) if bn_mode else None
        save_invstd = torch.empty(WT, dtype=torch.float32, device=dev) if bn_mode else None
        ws = torch.empty(max(L.cbl_pointwise_mlp_layers_workspace_bytes(_i(n), _i(n0), _i(K), _i(H), _i(C_out), _i(layers)), 1), dtype=torch.uint8, device=dev)
        _lib.check(L.cbl_pointwise_mlp_layers_forward(_i(n), _i(n0), _i(K), _i(H), _i(C_out), _lib.ptr(query_points), _lib.ptr(support_points),
                                                      _lib.ptr(neighbors_indices), _lib.ptr(center_term), _lib.ptr(neighbor_term), _lib.ptr(w_pos), _f(radius),
                                                      _i(layers), _lib.ptr(hidden_w), _i(bn_mode), _lib.ptr(gamma), _lib.ptr(beta), _f(eps), _f(momentum),
                                                      _lib.ptr(moving_mean), _lib.ptr(moving_variance), _i(act), _i(red), _lib.ptr(pad), _lib.ptr(save_mean),
                                                      _lib.ptr(save_invstd), _lib.ptr(out), _lib.ptr(ws), ctypes.c_size_t(ws.numel()), st),
                   "cbl_pointwise_mlp_layers_forward")
        ctx.save_for_backward(query_points, support_points, neighbors_indices, center_term, neighbor_term, w_pos, hidden_w, gamma, beta, save_mean,
                              save_invstd, pad, out)
        ctx.cfg = (radius, bn_mode, act, red, C_out, layers)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, s, idx, cen, nbr, wp, hw, gamma, beta, save_mean, save_invstd, pad, out = ctx.saved_tensors
        radius, bn_mode, act, red, C_out, layers = ctx.cfg
        n, K = idx.shape
        n0, H = nbr.shape
        grad_out = grad_out.contiguous()
        L = _lib.lib()
        dev = nbr.device
        st = _lib.stream_of(nbr)
        need = ctx.needs_input_grad
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        WT = layers * H + C_out
        gc = new(n, H) if cen is not None and need[3] else None
        gn = new(n0, H) if need[4] else None
        gwp = new(3, H) if wp is not None and need[5] else None
        ghw = new(hw.numel()) if need[6] else None
        gg = new(WT) if gamma is not None and need[7] else None
        gb = new(WT) if beta is not None and need[8] else None
        order = inv_start = inv_src = None
        if gn is not None:
            order, inv_start, inv_src = _pair_table(idx, n0, "pointwise_mlp")
        ws = torch.empty(max(L.cbl_pointwise_mlp_layers_workspace_bytes(_i(n), _i(n0), _i(K), _i(H), _i(C_out), _i(layers)), 1), dtype=torch.uint8, device=dev)
        _lib.check(L.cbl_pointwise_mlp_layers_backward_csr(_i(n), _i(n0), _i(K), _i(H), _i(C_out), _lib.ptr(q), _lib.ptr(s), _lib.ptr(idx), _lib.ptr(cen),
                                                           _lib.ptr(nbr), _lib.ptr(wp), _f(radius), _i(layers), _lib.ptr(hw), _i(bn_mode), _lib.ptr(gamma),
                                                           _lib.ptr(beta), _lib.ptr(save_mean), _lib.ptr(save_invstd), _i(act), _i(red), _lib.ptr(pad),
                                                           _lib.ptr(out), _lib.ptr(grad_out), _lib.ptr(order), _lib.ptr(inv_start), _lib.ptr(inv_src),
                                                           _lib.ptr(gc), _lib.ptr(gn), _lib.ptr(gwp), _lib.ptr(ghw), _lib.ptr(gg), _lib.ptr(gb), _lib.ptr(ws),
                                                           ctypes.c_size_t(ws.numel()), st), "cbl_pointwise_mlp_layers_backward_csr")
        gcen = _center_rows_to_support(gc, idx, n0, H, "pointwise_mlp") if gc is not None else None
        return (None, None, None, gcen, gn, gwp, ghw, gg, gb) + (None,) * 10


_PW_LAYERS_H = (16, 144)        # the hidden widths csrc/pointwise_mlp_layers.hip takes (one matrix tile .. half the ConvNet's widest bottleneck)


def _pw_layers_limits(fc_num, H, K=None):
    """refuses the depths, widths and neighbour counts the per-pair layer kernels do not cover, naming fc_num"""
    if fc_num < 1 or fc_num > 3:
        raise NotImplementedError("pointwisemlp.fc_num {}: fc_num 1, 2 and 3 are implemented".format(fc_num))
    if not _PW_LAYERS_H[0] <= H <= _PW_LAYERS_H[1]:
        raise NotImplementedError("pointwisemlp.fc_num {}: only fc_num 1 is implemented for hidden layers of width {} (the per-pair layer kernels take {} "
                                  "to {})".format(fc_num, H, *_PW_LAYERS_H))
    if K is not None and (K > 128 or (K > 48 and H > 64)):
        raise NotImplementedError("pointwisemlp.fc_num {}: {} neighbours with hidden layers of width {} (at most 48, or 128 up to width 64)".format(fc_num, K, H))


def pointwise_mlp(query_points, support_points, neighbors_indices, features, radius, weights, gamma=None, beta=None, moving_mean=None,
                  moving_variance=None, *, local_input_feature="dp_fj", reduction="max", activation_fn="relu", is_training=True, bn_momentum=0.98,
                  bn_eps=1e-3, fc_num=None, fc_hidden=()):
    """PointWiseMLP (n, out_fdim)  (tensorflow/models/local_aggregation_operators.py:503-617; options as config.pointwisemlp.*) with fc_num 1 + len(fc_hidden)
    (1, 2 or 3).  weights: the TF variable of the FIRST layer (D_in, width), rows in the concatenation order of :573-584 — fc_1/weights (D_in, C_out) for
    fc_num 1, fc_0/weights (D_in, H) with H = max(in_fdim // 2, 9) otherwise; gamma / beta: its batch norm (gamma None: bn=False); moving_mean /
    moving_variance: updated in place when training (TF convention), used when not.
    The first layer is linear in the concatenated blocks: y = dp @ W_p + (f @ (W_fi - W_df))[idx[:, 0]] + (f @ (W_df + W_fj))[idx] — the two per-point products
    are dense layers here (autograd carries the fold and the weight gradient), the per-pair part is csrc/pointwise_mlp.hip.
    fc_hidden: the layers behind the first, in order, each (weights (in, out), gamma, beta, moving_mean, moving_variance) with the last four None exactly
    when the first layer's gamma is None (:589-600: no layer has a bias, every layer its own batch norm over all n*K pair rows and the activation; the last
    one is (H, C_out)).  The per-pair part is then csrc/pointwise_mlp_layers.hip (16 <= H <= 144; K <= 48, or <= 128 up to H = 64).  fc_num None:
    1 + len(fc_hidden); a given fc_num that disagrees with the layers passed is refused.  With fc_hidden empty the call is fc_num 1's."""
    fc_hidden = tuple(fc_hidden)
    if fc_num is None:
        fc_num = 1 + len(fc_hidden)
    if fc_num != 1 + len(fc_hidden):
        raise NotImplementedError("pointwisemlp.fc_num {}: {} layer(s) were passed (weights and fc_hidden); fc_num 2 and 3 take the layers behind the first "
                                  "in fc_hidden".format(fc_num, 1 + len(fc_hidden)))
    if fc_hidden:
        _pw_layers_limits(fc_num, weights.shape[1], neighbors_indices.shape[1])
        for l, layer in enumerate(fc_hidden, 1):
            if len(layer) != 5:
                raise ValueError("fc_hidden[{}]: (weights, gamma, beta, moving_mean, moving_variance) expected".format(l - 1))
            if any((t is None) != (gamma is None) for t in layer[1:3]) or (gamma is None and any(t is not None for t in layer[3:])):
                raise ValueError("fc_hidden[{}]: batch-norm variables present on one layer and absent on another (one bn setting holds for every "
                                 "layer)".format(l - 1))
            H = weights.shape[1]
            if layer[0].dim() != 2 or layer[0].shape[0] != H or (l < len(fc_hidden) and layer[0].shape[1] != H):
                raise ValueError("fc_hidden[{}]: weights of shape {}, behind a layer of width {} it has ({}, {})".format(
                    l - 1, tuple(layer[0].shape), H, H, H if l < len(fc_hidden) else "out_fdim"))
            width = layer[0].shape[1]
            for t, name in zip(layer[1:], ("gamma", "beta", "moving_mean", "moving_variance")):
                if t is not None and tuple(t.shape) != (width,):
                    raise ValueError("fc_hidden[{}]: {} of shape {}, a layer of width {} has ({},)".format(l - 1, name, tuple(t.shape), width, width))
            _chk(layer[0], torch.float32, "fc_hidden[{}] weights".format(l - 1))
            for t, name in zip(layer[1:], ("gamma", "beta", "moving_mean", "moving_variance")):
                if t is not None:
                    _chk(t, torch.float32, "fc_hidden[{}] {}".format(l - 1, name))
    _chk(query_points, torch.float32, "query_points"); _chk(support_points, torch.float32, "support_points")
    _chk(neighbors_indices, torch.int32, "neighbors_indices"); _chk(features, torch.float32, "features")
    _chk(weights, torch.float32, "weights")
    for t, name in ((gamma, "gamma"), (beta, "beta"), (moving_mean, "moving_mean"), (moving_variance, "moving_variance")):
        if t is not None:
            _chk(t, torch.float32, name)
    if local_input_feature not in POINTWISE_MLP_INPUTS:
        raise NotImplementedError("local_input_feature {} not supported in Point-wise MLP".format(local_input_feature))
    if reduction not in _PW_REDUCTIONS:
        raise NotImplementedError("Reduction {} not supported in Point-wise MLP.".format(reduction))
    C, C_out, K = features.shape[1], (fc_hidden[-1][0] if fc_hidden else weights).shape[1], neighbors_indices.shape[1]
    has_dp, has_fi, has_fj = local_input_feature.startswith("dp"), "fi_df" in local_input_feature, local_input_feature.endswith("fj")
    if weights.shape[0] != 3 * has_dp + 2 * C * has_fi + C * has_fj:
        raise ValueError("weights: {} rows, local_input_feature {} of {} features has {}".format(weights.shape[0], local_input_feature, C,
                                                                                              3 * has_dp + 2 * C * has_fi + C * has_fj))
    if C_out % 4 != 0 or C_out > 1024:
        raise NotImplementedError("pointwise_mlp: out_fdim {} (a multiple of 4 up to 1024, for fc_num 1, 2 and 3)".format(C_out))
    if K > 128:
        raise NotImplementedError("pointwise_mlp: {} neighbours (at most 128)".format(K))
    if gamma is not None and not is_training and any(t is None for t in (moving_mean, moving_variance) + tuple(t for h in fc_hidden for t in h[3:])):
        raise ValueError("pointwise_mlp: is_training=False needs moving_mean and moving_variance")
    from . import dense
    o = 3 if has_dp else 0
    w_pos = weights[:3].contiguous() if has_dp else None
    center_term = None
    if has_fi:
        w_fi, w_df = weights[o:o + C], weights[o + C:o + 2 * C]
        o += 2 * C
        center_term = dense.linear(features, (w_fi - w_df).t())
        w_n = w_df + weights[o:o + C] if has_fj else w_df
    else:
        w_n = weights[o:o + C]
    neighbor_term = dense.linear(features, w_n.t())
    bn_mode = 0 if gamma is None else (1 if is_training else 2)
    if fc_hidden:
        layers, H = len(fc_hidden), weights.shape[1]
        hidden_w = torch.cat([h[0].reshape(-1) for h in fc_hidden])
        pack = lambda first, k: None if first is None else torch.cat([first] + [h[k] for h in fc_hidden])
        moving = [(moving_mean, moving_variance)] + [(h[3], h[4]) for h in fc_hidden]
        mm = mv = None
        if bn_mode and all(m is not None and v is not None for m, v in moving):
            with torch.no_grad():
                mm, mv = torch.cat([m for m, _ in moving]), torch.cat([v for _, v in moving])
        out = _PointWiseMLPLayers.apply(query_points, support_points, neighbors_indices, center_term, neighbor_term.contiguous(), w_pos, hidden_w,
                                        pack(gamma, 1), pack(beta, 2), mm, mv, float(radius), bn_mode, _PW_ACTIVATIONS.get(activation_fn, 0),
                                        _PW_REDUCTIONS[reduction], float(bn_momentum), float(bn_eps), C_out, layers)
        if bn_mode == 1 and mm is not None:                          # every layer's moving statistics, updated by the kernels in the packed buffer
            with torch.no_grad():
                o = 0
                for m, v in moving:
                    m.copy_(mm[o:o + m.numel()]); v.copy_(mv[o:o + v.numel()])
                    o += m.numel()
        return out
    return _PointWiseMLP.apply(query_points, support_points, neighbors_indices, center_term, neighbor_term.contiguous(), w_pos, gamma, beta, moving_mean,
                               moving_variance, float(radius), bn_mode, _PW_ACTIVATIONS.get(activation_fn, 0), _PW_REDUCTIONS[reduction],
                               float(bn_momentum), float(bn_eps))


class PointWiseMLP(torch.nn.Module):
    """the operator with its variables (TF names): `weights` (xavier), `gamma`, `beta` and the moving statistics of the first layer — fc_1 (D_in, out_fdim)
    for fc_num 1, fc_0 (D_in, H) with H = max(in_fdim // 2, 9) for fc_num 2 and 3 — and `weights_l`, `gamma_l`, `beta_l`, `moving_mean_l`,
    `moving_variance_l` of the layers l = 1 .. fc_num - 1 behind it ((H, H), the last one (H, out_fdim); :589-600)"""

    def __init__(self, in_fdim, out_fdim, local_input_feature="dp_fj", fc_num=1, reduction="max", activation_fn="relu", bn=True, bn_momentum=0.98,
                 bn_eps=1e-3):
        super().__init__()
        H = max(in_fdim // 2, 9)
        if fc_num != 1:
            _pw_layers_limits(fc_num, H)
        if local_input_feature not in POINTWISE_MLP_INPUTS:
            raise NotImplementedError("local_input_feature {} not supported in Point-wise MLP".format(local_input_feature))
        d_in = 3 * local_input_feature.startswith("dp") + 2 * in_fdim * ("fi_df" in local_input_feature) + in_fdim * local_input_feature.endswith("fj")
        self.local_input_feature, self.fc_num, self.reduction, self.activation_fn = local_input_feature, fc_num, reduction, activation_fn
        self.bn_momentum, self.bn_eps = bn_momentum, bn_eps
        ins = [d_in] + [H] * (fc_num - 1)
        outs = [H] * (fc_num - 1) + [out_fdim]
        for l, (i, o) in enumerate(zip(ins, outs)):
            tag = "" if l == 0 else "_{}".format(l)
            w = torch.nn.Parameter(torch.empty(i, o))
            torch.nn.init.xavier_uniform_(w)
            setattr(self, "weights" + tag, w)
            if bn:
                setattr(self, "gamma" + tag, torch.nn.Parameter(torch.ones(o)))
                setattr(self, "beta" + tag, torch.nn.Parameter(torch.zeros(o)))
                self.register_buffer("moving_mean" + tag, torch.zeros(o))
                self.register_buffer("moving_variance" + tag, torch.ones(o))
            else:
                for name in ("gamma", "beta", "moving_mean", "moving_variance"):
                    setattr(self, name + tag, None)

    def tf_scopes(self):
        """variable name -> the TF variable scope of its layer (:590-600): fc_0 .. fc_{fc_num-2} for the hidden layers, fc_{fc_num} for the last one — the
        number fc_num - 1 is skipped (fc_num 1: fc_1 alone), which someone loading a reference checkpoint has to know"""
        scope = lambda l: "fc_{}".format(l if l < self.fc_num - 1 else self.fc_num)
        names = {}
        for l in range(self.fc_num):
            tag = "" if l == 0 else "_{}".format(l)
            for name in ("weights", "gamma", "beta", "moving_mean", "moving_variance"):
                if getattr(self, name + tag) is not None:
                    names[name + tag] = scope(l)
        return names

    def forward(self, query_points, support_points, neighbors_indices, features, radius):
        hidden = [tuple(getattr(self, name + "_{}".format(l)) for name in ("weights", "gamma", "beta", "moving_mean", "moving_variance"))
                  for l in range(1, self.fc_num)]
        return pointwise_mlp(query_points, support_points, neighbors_indices, features, radius, self.weights, self.gamma, self.beta, self.moving_mean,
                             self.moving_variance, local_input_feature=self.local_input_feature, reduction=self.reduction,
                             activation_fn=self.activation_fn, is_training=self.training, bn_momentum=self.bn_momentum, bn_eps=self.bn_eps,
                             fc_num=self.fc_num, fc_hidden=hidden)


def _ind_max_pool_forward(x, inds):
    """-> out (n2, d), scratch (d): the column minima of x as ordered keys, which the gradient reads"""
    n1, d = x.shape
    n2, k = inds.shape
    scratch = torch.empty(d, dtype=torch.int32, device=x.device)
    out = torch.empty((n2, d), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().cbl_ind_max_pool(_i(n1), _i(n2), _i(k), _i(d), _lib.ptr(x), _lib.ptr(inds), _lib.ptr(scratch), _lib.ptr(out), _lib.stream_of(x)),
               "cbl_ind_max_pool")
    return out, scratch


def _ind_closest_pool_forward(x, inds):
    n1, d = x.shape
    n2, k = inds.shape
    out = torch.empty((n2, d), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().cbl_ind_closest_pool(_i(n1), _i(n2), _i(k), _i(d), _lib.ptr(x), _lib.ptr(inds), _lib.ptr(out), _lib.stream_of(x)),
               "cbl_ind_closest_pool")
    return out


class _IndMaxPool(Function):
    """cbl_ind_max_pool and its gradient csrc/index_pool.hip (cbl_amd.h): reduce_max / reduce_min share a gradient equally among ties"""

    @staticmethod
    def forward(ctx, x, inds):
        out, scratch = _ind_max_pool_forward(x, inds)
        ctx.save_for_backward(x, inds, scratch, out)                     # scratch is kept instead of discarded
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, inds, scratch, out = ctx.saved_tensors
        n1, d = x.shape
        n2, k = inds.shape
        grad_out = grad_out.contiguous()
        L = _lib.lib()
        from . import pointops
        # always the gather over the transposed table: the atomic cbl_grouping_backward does not guard shadow ids, and ties need the table's pairs anyway
        tr = pointops.neighbor_transpose(inds, n1, build=True)
        if tr is None:
            raise NotImplementedError(_NO_TABLE.format("ind_max_pool"))
        order, inv_start, inv_src = tr
        grad_x = torch.empty_like(x)
        ws = torch.empty(max(L.cbl_ind_max_pool_backward_workspace_bytes(_i(n1), _i(n2), _i(k), _i(d)), 1), dtype=torch.uint8, device=x.device)
        _lib.check(L.cbl_ind_max_pool_backward_csr(_i(n1), _i(n2), _i(k), _i(d), _lib.ptr(x), _lib.ptr(inds), _lib.ptr(scratch), _lib.ptr(out), _lib.ptr(grad_out),
                                                   _lib.ptr(order), _lib.ptr(inv_start), _lib.ptr(inv_src), _lib.ptr(grad_x), _lib.ptr(ws),
                                                   ctypes.c_size_t(ws.numel()), _lib.stream_of(x)), "cbl_ind_max_pool_backward_csr")
        return grad_x, None


_first_columns = collections.OrderedDict()     # neighbour table -> (the table, its contiguous first column), the 16 most recent


def first_column(inds):
    """inds[:, :1] as a tensor of its own, the SAME one for the same table from call to call: the transposed table built for it (neighbor_state's registry,
    keyed by the tensor) is then found again by every later backward pass instead of being built per call"""
    if inds.shape[1] == 1:
        return inds
    from . import neighbor_state
    version = neighbor_state._version_of(inds)
    if version < 0:
        return inds[:, :1].contiguous()
    key = (inds.data_ptr(), tuple(inds.shape), version, inds.device)
    ent = _first_columns.get(key)
    if ent is None:
        ent = _first_columns[key] = (inds, inds[:, :1].contiguous())       # holding the table keeps its address from being reused under the key
        while len(_first_columns) > 16:
            _first_columns.popitem(last=False)
    else:
        _first_columns.move_to_end(key)
    return ent[1]


class _IndClosestPool(Function):
    """cbl_ind_closest_pool; its gradient is the row scatter through the first column, as a gather over that column's transposed table"""

    @staticmethod
    def forward(ctx, x, inds):
        out = _ind_closest_pool_forward(x, inds)
        ctx.save_for_backward(first_column(inds))
        ctx.shape = tuple(x.shape)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        inds0, = ctx.saved_tensors
        n1, d = ctx.shape
        grad_out = grad_out.contiguous()
        from . import pointops
        tr = pointops.neighbor_transpose(inds0, n1, build=True)          # shadow ids are in no segment: they receive nothing
        if tr is None:
            raise NotImplementedError(_NO_TABLE.format("ind_closest_pool"))
        grad_x = torch.empty((n1, d), dtype=torch.float32, device=grad_out.device)
        _lib.check(_lib.lib().cbl_grouping_backward_csr_rows(_i(n1), _i(d), _i(d), _i(0), _lib.ptr(grad_out), _lib.ptr(tr[0]), _lib.ptr(tr[1]), _lib.ptr(tr[2]),
                                                             _lib.ptr(grad_x), _lib.stream_of(grad_out)), "cbl_grouping_backward_csr_rows")
        return grad_x, None


def ind_max_pool(x, inds):
    """basic_operators.py:155-172, differentiable in x (ties of the maximum and of the shadow row's column minimum share the gradient equally, as
    tf.reduce_max / tf.reduce_min do)"""
    _chk(x, torch.float32, "x"); _chk(inds, torch.int32, "inds")
    if not (x.requires_grad and torch.is_grad_enabled()):                # no gradient asked for: the forward entry alone, nothing kept
        return _ind_max_pool_forward(x, inds)[0]
    return _IndMaxPool.apply(x, inds)


def ind_closest_pool(x, inds):
    """basic_operators.py:175-192, differentiable in x"""
    _chk(x, torch.float32, "x"); _chk(inds, torch.int32, "inds")
    if not (x.requires_grad and torch.is_grad_enabled()):
        return _ind_closest_pool_forward(x, inds)
    return _IndClosestPool.apply(x, inds)


def nearest_upsample(features, upsample_inds):
    """nearest_upsample_block (models/heads/seg_head.py:13-28): features (n1, d) of the coarser layer, upsample_inds (n2, max_num) -> (n2, d)"""
    return ind_closest_pool(features, upsample_inds)
