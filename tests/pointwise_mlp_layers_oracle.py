"""TEST ORACLE: PointWiseMLP with fc_num 2 and 3 (tensorflow/models/local_aggregation_operators.py:503-617) restated in float64 torch in the reference's DIRECT
form — gather the neighbourhoods, concatenate the blocks of `local_input_feature` (:573-584), then per layer `@ W` (no bias), batch norm over all n*K pair
rows, shadow rows included (tf.layers.batch_normalization: biased variance, moving = moving * momentum + batch * (1 - momentum)), activation
(batch_conv1d_1x1, basic_operators.py:243-289): fc_0 .. fc_{fc_num-2} of width H = max(C // 2, 9) (:589), then fc_{fc_num} of width C_out; mask, reduction.
Gradients by autograd; `amax` shares the gradient of a maximum among the entries that attain it, as tf.reduce_max does.  It uses neither the fold of the
first layer into per-point terms nor anything of the kernels (csrc/pointwise_mlp_layers.hip): kernel and oracle are independent formulations.  TensorFlow
itself is absent, so this is a restatement of the graph code, not a recording of it."""
import numpy as np
import torch

from tests import pointwise_mlp_oracle as P

MODES = P.MODES
REDUCTIONS = P.REDUCTIONS
ACTIVATIONS = P.ACTIVATIONS
FC_NUMS = (2, 3)
BNS = ("batch", "moving", None)
BASE = (96, 48, 10, 32, 32)                                          # n0, n, K, C (H = 16), C_out
close = P.close

# seeds at BASE on which no relu of any layer and no arg-max can flip between fp32 and float64, for every reduction and every bn mode (found on the CPU with
# find_seed below; asserted again by every case that uses them)
SEEDS = {(2, "dp_fj"): 8, (2, "fi_df"): 9, (2, "dp_fi_df"): 1, (2, "dp_fi_df_fj"): 1,
         (3, "dp_fj"): 1, (3, "fi_df"): 3, (3, "dp_fi_df"): 2, (3, "dp_fi_df_fj"): 7}
# the same at BASE with features of mean 8, for ('max', 'relu') with batch statistics
SEEDS_MEAN_8 = {(2, "dp_fj"): 0, (2, "dp_fi_df_fj"): 0, (3, "dp_fj"): 0, (3, "dp_fi_df_fj"): 0}
# width and tile edges (n0, n, K, C, C_out): H = 18 (no multiple of 16 or 4); C = C_out = 72; H = 144 at K = 48 with C_out = 288; H = 64 at K = 128; one float4 of
# output columns; one neighbour; one query; n K = 500 (no multiple of 16).  The two largest with few queries: the same tiles and LDS plans, several trips
SHAPES = [(96, 48, 10, 36, 32), (96, 48, 10, 72, 72), (160, 5, 48, 288, 288), (160, 5, 128, 128, 32), (96, 48, 10, 32, 4), (96, 48, 1, 32, 32),
          (96, 1, 10, 32, 32), (96, 50, 10, 32, 32)]
HUB = (8, 300, 3, 32, 32)                                             # support point 0 owns 300 pairs: more than the 256 rows a tile can have
# more trips than every grid cap (PLM_F_BLOCKS, PLM_BQ_BLOCKS, PLM_BT_BLOCKS = 512 of the kernel file) at H = 16, C_out = 4, K = 4.  The kernels' LDS plan gives a
# forward trip 48 queries with one hidden layer and 32 with two (24 600 queries: 513 and 769 trips), a query-side backward trip 32 and 24 (769 and 1025
# trips), a target-side trip 10 and 16 targets (8 300 targets: 830 and 519 trips)
CAPS = (8300, 24600, 4, 32, 4)


def hidden_width(C):
    return max(C // 2, 9)                                            # :589


def widths(C, C_out, fc_num):
    return [hidden_width(C)] * (fc_num - 1) + [C_out]


def _layers(case, rng, C, C_out, fc_num, D):
    """weights and batch-norm variables of every layer: W[0] (D_in, H), W[l] (H, H), W[-1] (H, C_out), TF's (in, out) order"""
    ws = widths(C, C_out, fc_num)
    ins = [D] + ws[:-1]
    case["W"] = [(rng.normal(size=(i, o)) / np.sqrt(i)).astype(np.float32) for i, o in zip(ins, ws)]
    case["gamma"] = [rng.uniform(0.5, 1.5, o).astype(np.float32) for o in ws]
    case["beta"] = [rng.normal(0, 0.3, o).astype(np.float32) for o in ws]
    case["moving_mean"] = [rng.normal(0, 0.5, o).astype(np.float32) for o in ws]
    case["moving_var"] = [rng.uniform(0.5, 2.0, o).astype(np.float32) for o in ws]
    case["fc_num"] = fc_num
    return case


def make_case(n0, n, K, C, C_out, seed, mode, fc_num, offset=0.0, pad_frac=0.3, all_shadow_row=True, padding=True):
    """the scene of pointwise_mlp_oracle.make_case (support points in the unit cube, the K nearest as neighbours, up to pad_frac trailing shadow entries per
    row, query 0 without any neighbour; features of mean `offset`) with the layers of fc_num 2 or 3"""
    base = P.make_case(n0, n, K, C, 4, seed, mode, offset=offset, pad_frac=pad_frac, all_shadow_row=all_shadow_row, padding=padding)
    rng = np.random.default_rng(1000 + seed)
    case = dict(q=base["q"], s=base["s"], idx=base["idx"], f=base["f"], mode=mode, radius=P.RADIUS)
    case["go"] = rng.normal(size=(n, C_out)).astype(np.float32)
    return _layers(case, rng, C, C_out, fc_num, P.d_in(mode, C))


def random_case(n0, n, K, C, C_out, seed, mode, fc_num, hub=False, pad_frac=0.3):
    """neighbours drawn at random (no distance matrix: any size); hub: column 0 of every query is support point 0, which then owns n pairs"""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0, 1, (n0, 3)).astype(np.float32)
    q = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    idx = rng.integers(0, n0, (n, K)).astype(np.int32)
    if hub:
        idx[:, 0] = 0
    npad = rng.integers(0, int(K * pad_frac) + 1, n)
    for i in np.nonzero(npad)[0]:
        idx[i, K - npad[i]:] = n0
    if not hub:
        idx[0, :] = n0
    case = dict(q=q, s=s, idx=np.ascontiguousarray(idx), f=rng.normal(size=(n0, C)).astype(np.float32), mode=mode, radius=0.5)
    case["go"] = rng.normal(size=(n, C_out)).astype(np.float32)
    return _layers(case, rng, C, C_out, fc_num, P.d_in(mode, C))


def direct(q, s, idx, f, W, gamma, beta, radius, mode, reduction, activation, bn="batch", moving_mean=None, moving_var=None, eps=1e-3):
    """-> out (n, C_out), [z_l (n, K, width_l)] pre-activations, a (n, K, C_out) activation * mask, [batch mean_l], [biased batch variance_l],
    null (n, K): the pairs whose concatenated input is exactly zero, [xhat_l]"""
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
    x = torch.cat(blocks, -1)
    null = (x.detach() == 0).all(-1)
    zs, xhs, means, variances = [], [], [], []
    for l in range(len(W)):
        y = x @ W[l]
        mean = y.mean((0, 1))
        var = y.var((0, 1), unbiased=False)
        if bn == "batch":
            xh = (y - mean) / torch.sqrt(var + eps)
        elif bn == "moving":
            xh = (y - moving_mean[l]) / torch.sqrt(moving_var[l] + eps)
        else:
            xh = y
        z = xh * gamma[l] + beta[l] if bn else xh
        z.retain_grad()
        xhs.append(xh.detach())
        x = torch.relu(z) if activation == "relu" else torch.nn.functional.leaky_relu(z, 0.2) if activation == "leaky_relu" else z
        zs.append(z); means.append(mean); variances.append(var)
    a = x * (idx < n0).to(x.dtype)[..., None]
    if reduction == "max":
        out = a.amax(1)
    elif reduction == "sum":
        out = a.sum(1)
    else:
        nn_ = (idx < idx.max()).to(x.dtype).sum(-1, keepdim=True) + 1e-5
        out = a.sum(1) / nn_
    return out, zs, a, means, variances, null, xhs


def reference(case, reduction, activation, bn="batch", momentum=0.98, eps=1e-3, backward=True):
    """float64 results of one case: out; under grad_out = case['go'] the gradients grad_f, grad_W / grad_gamma / grad_beta (a list over the layers each); the
    updated moving statistics of every layer; and the figures of the flip precondition: min_abs_z = the smallest |z_l| over ALL pairs of every hidden layer
    and over the valid pairs of the last one — but for a z_l that is exactly 0 on a pair whose input is exactly zero ('fi_df' without batch norm on a query
    whose neighbours are all shadow: every product is 0 in fp32 as in float64, so nothing can flip there) —, min_gap = (for 'max') the smallest
    gap between the best and the second-best value of a row whose best is positive"""
    t = lambda a, g=False: torch.tensor(a, dtype=torch.float64 if a.dtype.kind == "f" else torch.int64, requires_grad=g)
    f = t(case["f"], True)
    W = [t(w, True) for w in case["W"]]
    gamma = [t(g, True) for g in case["gamma"]]
    beta = [t(b, True) for b in case["beta"]]
    out, zs, a, means, variances, null, xhs = direct(t(case["q"]), t(case["s"]), t(case["idx"]), f, W, gamma, beta, case["radius"], case["mode"], reduction, activation,
                                          bn, [t(m) for m in case["moving_mean"]], [t(v) for v in case["moving_var"]], eps)
    res = dict(out=out.detach().numpy())
    if backward:
        out.backward(t(case["go"]))
        g = lambda x, like: x.grad.numpy() if x.grad is not None else np.zeros(like.shape, np.float64)
        res.update(grad_f=g(f, case["f"]), grad_W=[g(w, c) for w, c in zip(W, case["W"])],
                   grad_gamma=[g(x, c) for x, c in zip(gamma, case["gamma"])], grad_beta=[g(x, c) for x, c in zip(beta, case["beta"])])
        # the sums of the magnitudes of the terms of grad_beta_l = sum dz_l and grad_gamma_l = sum dz_l xhat_l over the n K pair rows (see close_sum)
        # — times sqrt(m) below the last layer, where every term dz_l is itself an inner product of m = the next layer's width fp32 products
        depth = [float(np.sqrt(w.shape[1])) for w in case["W"][1:]] + [1.0]
        res["beta_total"] = [float(z.grad.abs().sum((0, 1)).max()) * d for z, d in zip(zs, depth)]
        res["gamma_total"] = [float((z.grad * xh).abs().sum((0, 1)).max()) * d for z, xh, d in zip(zs, xhs, depth)]
    res["moving_mean"] = [m.astype(np.float64) * momentum + b.detach().numpy() * (1 - momentum) for m, b in zip(case["moving_mean"], means)]
    res["moving_var"] = [m.astype(np.float64) * momentum + b.detach().numpy() * (1 - momentum) for m, b in zip(case["moving_var"], variances)]
    valid = case["idx"] < case["f"].shape[0]
    exact = lambda z: null.numpy()[..., None] & (z == 0)
    lows = []
    for z in zs[:-1]:
        z = z.detach().numpy()
        z = np.abs(z[~exact(z)])
        lows.append(float(z.min()) if z.size else np.inf)
    last = zs[-1].detach().numpy()[valid]
    lows.append(float(np.abs(last).min()) if last.size else np.inf)
    res["min_abs_z"] = min(lows)
    res["min_gap"] = np.inf
    if reduction == "max" and a.shape[1] > 1:
        top = np.sort(a.detach().numpy(), 1)[:, -2:, :]
        gap = (top[:, 1] - top[:, 0])[top[:, 1] > 0]
        res["min_gap"] = float(gap.min()) if gap.size else np.inf
    return res


def flip_free(ref, reduction, activation):
    ok = True
    if activation != "none" or reduction == "max":
        ok = ok and ref["min_abs_z"] >= 1e-5
    if reduction == "max":
        ok = ok and ref["min_gap"] >= 5e-5
    return ok


def assert_flip_free(ref, reduction, activation):
    """a relu or arg-max flip between fp32 and float64 is not a kernel error: gradient cases with an activation or 'max' run on seeds where none can occur"""
    if activation != "none" or reduction == "max":
        assert ref["min_abs_z"] >= 1e-5, "bad seed: a pre-activation within 1e-5 of zero (%.2e)" % ref["min_abs_z"]
    if reduction == "max":
        assert ref["min_gap"] >= 5e-5, "bad seed: two candidates of a maximum within 5e-5 (%.2e)" % ref["min_gap"]


def close_sum(got, ref, total, what=""):
    """the contract for an array that is a SUM over the n K pair rows: 1e-4 relative; absolute 1e-4 * max|ref|, or where that is larger one fp32 unit
    (2^-23) of `total` = the sum of the terms' magnitudes.  The contract measures an error against the array's own magnitude, which for a sum that cancels
    is not max|ref|: with the identity as activation and batch statistics, sum dz_l of a hidden layer is zero in exact arithmetic (beta_l shifts y_{l+1} by
    a constant, which the next batch norm removes); the float64 reference holds its own rounding noise there (1e-13) and 1e-4 * max|ref| would ask the fp32
    result for more digits than float64 has.  Every term of the sum carries factors held in fp32 (the two coefficients of the batch-norm backward, gamma *
    invstd), so the sum cannot be known better than one fp32 unit of the sum of its terms' magnitudes, however it is accumulated; below the last layer
    a term is itself an inner product of m fp32 products (m = the next layer's width), known to about sqrt(m) units of its own magnitude, and `total`
    carries that factor.  Where a sum does not
    cancel the contract's own bound is the larger one (at n K = 98 400 still by a factor 2.7 for terms of random sign)."""
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=max(1e-4 * float(np.abs(ref).max()), 2.0 ** -23 * total, 1e-34), err_msg=what)


def find_seed(make, configs, seeds=range(64)):
    """the first seed whose case make(seed) is flip-free under every (reduction, activation, bn) of `configs`"""
    for seed in seeds:
        case = make(seed)
        if all(flip_free(reference(case, r, a, bn, backward=False), r, a) for r, a, bn in configs):
            return seed
    raise AssertionError("no flip-free seed")


def base_case(fc_num, mode):
    return make_case(*BASE, SEEDS[(fc_num, mode)], mode, fc_num)


def check(res, ref, bn="batch", what=""):
    """out, every gradient, and in batch mode every layer's moving statistics, within the 1e-4 contract"""
    close(res["out"], ref["out"], what + " out")
    if "grad_f" in res:
        close(res["grad_f"], ref["grad_f"], what + " grad features")
        for l, (got, want) in enumerate(zip(res["grad_W"], ref["grad_W"])):
            close(got, want, "%s grad weights of layer %d" % (what, l))
        if bn:
            for l in range(len(ref["grad_gamma"])):
                close_sum(res["grad_gamma"][l], ref["grad_gamma"][l], ref["gamma_total"][l], "%s grad gamma of layer %d" % (what, l))
                close_sum(res["grad_beta"][l], ref["grad_beta"][l], ref["beta_total"][l], "%s grad beta of layer %d" % (what, l))
    if bn == "batch" and "moving_mean" in res:
        for l in range(len(ref["moving_mean"])):
            close(res["moving_mean"][l], ref["moving_mean"][l], "%s moving mean of layer %d" % (what, l))
            close(res["moving_var"][l], ref["moving_var"][l], "%s moving variance of layer %d" % (what, l))


if __name__ == "__main__":                                           # python -m tests.pointwise_mlp_layers_oracle: the SEEDS table
    full = [(r, "relu", bn) for r in ("sum", "mean", "max") for bn in BNS] + [("max", "leaky_relu", "batch")]
    for fc_num in FC_NUMS:
        for mode in MODES:
            print((fc_num, mode), find_seed(lambda s: make_case(*BASE, s, mode, fc_num), full))
    for key in SEEDS_MEAN_8:
        print("mean 8", key, find_seed(lambda s: make_case(*BASE, s, key[1], key[0], offset=8.0), [("max", "relu", "batch")]))
