"""TEST ORACLE: PointWiseMLP (tensorflow/models/local_aggregation_operators.py:503-617, fc_num 1) restated in float64 torch in the reference's DIRECT form —
gather the neighbourhoods, concatenate the blocks of `local_input_feature` (:573-584), multiply by the (D_in, C_out) weights of `fc_1`, batch norm over all
n*K pairs (tf.layers.batch_normalization: biased variance, moving = moving * momentum + batch * (1 - momentum)), activation, mask, reduction.  Gradients by
autograd; `amax` shares the gradient of a maximum among the entries that attain it, as tf.reduce_max does.  It does NOT use the fold of the weights into
per-point terms that the kernels use (csrc/pointwise_mlp.hip): kernel and oracle are independent formulations.  TensorFlow itself is absent, so this is a
restatement of the graph code, not a recording of it."""
import numpy as np
import torch

MODES = ("dp_fj", "fi_df", "dp_fi_df", "dp_fi_df_fj")
REDUCTIONS = {"sum": 0, "mean": 1, "max": 2}
ACTIVATIONS = {"none": 0, "relu": 1, "leaky_relu": 2}
RADIUS = 0.15


def d_in(mode, C):
    return {"dp_fj": 3 + C, "fi_df": 2 * C, "dp_fi_df": 3 + 2 * C, "dp_fi_df_fj": 3 + 3 * C}[mode]


def make_case(n0, n, K, C, C_out, seed, mode, offset=0.0, pad_frac=0.3, all_shadow_row=True, padding=True):
    """a scene: support points in the unit cube, queries near some of them, the K nearest as neighbours with up to pad_frac trailing shadow entries (== n0)
    per row, query 0 without any neighbour (all_shadow_row); padding=False: no shadow entry anywhere (the 'mean' quirk: the largest REAL index then counts
    as padding in nn).  Features of mean `offset`."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0, 1, (n0, 3)).astype(np.float32)
    q = (s[rng.choice(n0, n, replace=False)] + rng.normal(0, 0.01, (n, 3))).astype(np.float32)
    d = ((s[None] - q[:, None]) ** 2).sum(-1)
    idx = np.argsort(d, 1)[:, :K].astype(np.int32)
    npad = rng.integers(0, int(K * pad_frac) + 1, n)
    if padding:
        for i in range(n):
            if npad[i]:
                idx[i, K - npad[i]:] = n0
        if all_shadow_row:
            idx[0, :] = n0
    f = (rng.normal(size=(n0, C)) + offset).astype(np.float32)
    D = d_in(mode, C)
    W = (rng.normal(size=(D, C_out)) / np.sqrt(D)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, C_out).astype(np.float32)
    beta = rng.normal(0, 0.3, C_out).astype(np.float32)
    go = rng.normal(size=(n, C_out)).astype(np.float32)
    mm = rng.normal(0, 0.5, C_out).astype(np.float32)
    mv = rng.uniform(0.5, 2.0, C_out).astype(np.float32)
    return dict(q=q, s=s, idx=np.ascontiguousarray(idx), f=f, W=W, gamma=gamma, beta=beta, go=go, moving_mean=mm, moving_var=mv, mode=mode, radius=RADIUS)


def direct(q, s, idx, f, W, gamma, beta, radius, mode, reduction, activation, bn="batch", moving_mean=None, moving_var=None, eps=1e-3):
    """-> out (n, C_out), z (n, K, C_out) pre-activation, a (n, K, C_out) activation * mask, batch mean, biased batch variance; float64 tensors.
    bn: 'batch' | 'moving' | None"""
    n0, C = f.shape
    n, K = idx.shape
    idx = idx.long()
    sf = torch.cat([f, torch.zeros_like(f[:1])])
    sp = torch.cat([s, torch.zeros_like(s[:1])])
    fj = sf[idx]
    fi = sf[idx[:, :1]].expand(-1, K, -1)
    df = fj - fi
    dp = (sp[idx] - q[:, None]) / radius
    blocks = {"dp_fj": [dp, fj], "fi_df": [fi, df], "dp_fi_df": [dp, fi, df], "dp_fi_df_fj": [dp, fi, df, fj]}[mode]
    y = torch.cat(blocks, -1) @ W
    mean = y.mean((0, 1))
    var = y.var((0, 1), unbiased=False)
    if bn == "batch":
        z = (y - mean) / torch.sqrt(var + eps) * gamma + beta
    elif bn == "moving":
        z = (y - moving_mean) / torch.sqrt(moving_var + eps) * gamma + beta
    else:
        z = y
    a = torch.relu(z) if activation == "relu" else torch.nn.functional.leaky_relu(z, 0.2) if activation == "leaky_relu" else z
    a = a * (idx < n0).to(y.dtype)[..., None]
    if reduction == "max":
        out = a.amax(1)
    elif reduction == "sum":
        out = a.sum(1)
    else:
        nn_ = (idx < idx.max()).to(y.dtype).sum(-1, keepdim=True) + 1e-5
        out = a.sum(1) / nn_
    return out, z, a, mean, var


def reference(case, reduction, activation, bn="batch", momentum=0.98, eps=1e-3):
    """float64 results of one case: out, gradients of (f, W, gamma, beta) under grad_out = case['go'], the updated moving statistics, and the two figures of
    the flip precondition: the smallest |z| over valid pairs and (for 'max') the smallest gap between the best and the second-best value of a row whose
    best is positive"""
    t = lambda a, g=False: torch.tensor(a, dtype=torch.float64 if a.dtype.kind == "f" else torch.int64, requires_grad=g)
    f, W, gamma, beta = t(case["f"], True), t(case["W"], True), t(case["gamma"], True), t(case["beta"], True)
    idx = t(case["idx"])
    out, z, a, mean, var = direct(t(case["q"]), t(case["s"]), idx, f, W, gamma, beta, case["radius"], case["mode"], reduction, activation, bn,
                                  t(case["moving_mean"]), t(case["moving_var"]), eps)
    out.backward(t(case["go"]))
    zero = np.zeros_like
    res = dict(out=out.detach().numpy(), grad_f=f.grad.numpy(), grad_W=W.grad.numpy(),
               grad_gamma=gamma.grad.numpy() if gamma.grad is not None else zero(case["gamma"], np.float64),
               grad_beta=beta.grad.numpy() if beta.grad is not None else zero(case["beta"], np.float64))
    res["moving_mean"] = case["moving_mean"].astype(np.float64) * momentum + mean.detach().numpy() * (1 - momentum)
    res["moving_var"] = case["moving_var"].astype(np.float64) * momentum + var.detach().numpy() * (1 - momentum)
    valid = case["idx"] < case["f"].shape[0]
    zz = z.detach().numpy()[valid]
    res["min_abs_z"] = float(np.abs(zz).min()) if zz.size else np.inf
    res["min_gap"] = np.inf
    if reduction == "max" and a.shape[1] > 1:
        top = np.sort(a.detach().numpy(), 1)[:, -2:, :]
        gap = (top[:, 1] - top[:, 0])[top[:, 1] > 0]
        res["min_gap"] = float(gap.min()) if gap.size else np.inf
    return res


def assert_flip_free(ref, reduction, activation):
    """a ReLU or arg-max flip between fp32 and float64 is not a kernel error: gradient cases with an activation or 'max' run on seeds where none can occur"""
    if activation != "none" or reduction == "max":
        assert ref["min_abs_z"] >= 1e-5, "bad seed: a pre-activation within 1e-5 of zero (%.2e)" % ref["min_abs_z"]
    if reduction == "max":
        assert ref["min_gap"] >= 5e-5, "bad seed: two candidates of a maximum within 5e-5 (%.2e)" % ref["min_gap"]


def close(got, ref, what=""):
    """the project's contract: 1e-4 relative, 1e-4 * max|ref| absolute"""
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4 * max(float(np.abs(ref).max()), 1e-30), err_msg=what)
