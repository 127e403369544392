"""TEST ORACLE: the batch norm + activation behind every local aggregation of the ConvNet (tensorflow/models/local_aggregation_operators.py:232-249 and its
siblings: batch_norm(..., scope='pool_bn') = tf.layers.batch_normalization as basic_operators.batch_norm sets it up, then relu / leaky_relu(0.2)) restated in
float64 torch in the DIRECT form under autograd: mean and biased variance over all rows (tf.nn.moments), moving = moving * momentum + batch * (1 - momentum).
It uses nothing of the kernels (csrc/pool_bn.hip): no pivots, no partial statistics, no hand-written gradient.  TensorFlow itself is absent, so — as for the
rest of a14 / a15 — this is a restatement of the graph code, not a recording of it: parity is unpinned by execution.

The contract is the project's 1e-4 of a column's scale (tests/unary_layer_oracle.py takes scale as max|ref| of the array; here every COLUMN is held to its own
maximum, which asks more): `close_columns`.  grad_gamma and grad_beta are sums over the rows and are held, per column, to the unary oracle's `close_sum` rule
with the total of their terms' magnitudes.  Two allowances are derived where they are used and hold for any float32 implementation: an entry of grad_x that
CANCELS is measured against the magnitudes of its terms (`terms`), and what the float32 rounding of the column's MEAN alone accounts for is added per column
(`floors`: negligible unless |mean| / std is large or two rows nearly coincide).  Gradient cases with relu or leaky_relu run on seeds where no
pre-activation lies within 1e-5 of zero."""
import numpy as np
import torch

from tests import unary_layer_oracle as U

ACTIVATIONS = U.ACTIVATIONS
BNS = U.BNS
close_sum = U.close_sum

# the kernels' constants (csrc/pool_bn.hip), named here so that the shapes below say what they cross
PB_BLOCK, PB_BATCH, PB_SLAB, PB_SMALL_SLAB, PB_MAX_CHUNKS, PB_SMALL_ROWS = 256, 8, 64, 8, 512, 512


def row_lanes(C, small):
    """the row lanes of a workgroup at width C (pb_geom)"""
    ncg, max_w = (C + 3) // 4, PB_SMALL_SLAB if small else PB_SLAB
    slabs = (ncg + max_w - 1) // max_w
    return PB_BLOCK // ((ncg + slabs - 1) // slabs)


def rows_past_the_cap(C):
    """the fewest rows at which the chunked kernels (statistics, sums and both element passes share ONE grid, (chunks, slabs), whose only cap is
    PB_MAX_CHUNKS) hold more than one fetch of PB_BATCH rows per row lane in a chunk — plus a ragged tail"""
    return PB_MAX_CHUNKS * row_lanes(C, False) * PB_BATCH + 70


# (rows, C).  rows 1, 2, 63, 64, 65 against every width class; PB_SMALL_ROWS and PB_SMALL_ROWS + 1: the two sides of the single-launch rule (at C = 72:
# 3 slabs of 6 column groups x 42 row lanes on the one side, 1 slab of 18 x 14 on the other); C = 1, 3 (never 16-byte aligned rows), 4, 72, 100 (a
# ragged 7-group slab in the single launch), 1152 (five slabs of 58 groups when chunked) and 4096 (16 slabs), each with a small counterpart
SHAPES = [(1, 1), (2, 3), (63, 4), (64, 72), (65, 100), (1, 1152), (2, 4096), (65, 1152), (63, 4096), (150, 72), (PB_SMALL_ROWS, 72),
          (PB_SMALL_ROWS + 1, 72), (PB_SMALL_ROWS + 1, 3), (1100, 1152), (1030, 4096), (3000, 100)]
CAP_SHAPES = [(rows_past_the_cap(4), 4), (rows_past_the_cap(100), 100)]
BASE = (150, 72)
SEED = 0                                                              # flip-free at BASE under every bn mode (python -m tests.pool_bn_oracle)


def make_case(rows, C, seed, mean=0.0, std=1.0, constant_column=None):
    """x (rows, C), gamma, beta, the moving statistics and grad_out `go`.  mean / std: every column is mean * std_c + std_c * normal, std_c in [0.5 std, 1.5
    std] — |mean| / std of the columns is `mean`.  constant_column: that column of x is one value"""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    sc = rng.uniform(0.5, 1.5, C) * std
    x = f32((rng.normal(size=(rows, C)) + mean * np.where(rng.random(C) < 0.5, -1.0, 1.0)) * sc)
    if constant_column is not None:
        x[:, constant_column] = x[0, constant_column]
    return dict(x=x, gamma=f32(rng.uniform(0.5, 1.5, C)), beta=f32(rng.normal(0, 0.3, C)), moving_mean=f32(rng.normal(0, 0.5, C)),
                moving_var=f32(rng.uniform(0.5, 2.0, C)), go=f32(rng.normal(size=(rows, C))))


RATIOS = (1.0, 1e2, 1e3, 1e4)


def ill_case(rows, C, seed):
    """columns with |mean| / std of 1, 1e2, 1e3, 1e4 in turn, and column 5 exactly constant at a large value"""
    case = make_case(rows, C, seed)
    rng = np.random.default_rng(seed + 100)
    ratio = np.array([RATIOS[c % 4] for c in range(C)])
    std = rng.uniform(0.5, 1.5, C)
    x = (rng.normal(size=(rows, C)) + ratio * np.where(rng.random(C) < 0.5, -1.0, 1.0)) * std
    x[:, 5] = 12345.678
    case["x"] = np.ascontiguousarray(x, np.float32)
    return case


def reference(case, bn="batch", activation="relu", momentum=0.98, eps=1e-3, backward=True, uncentred=False, dtype=torch.float64):
    """float64 results: out; under grad_out = case['go'] the three gradients; the updated moving statistics; mean / invstd; min_abs_z (the flip
    precondition) and the totals of the terms' magnitudes of the two column sums (close_sum).
    uncentred (with dtype=torch.float32): the variance as E[x^2] - E[x]^2 — NOT what the kernels do; tests/test_pool_bn_host.py substitutes it once to
    show that the ill-conditioned cases tell the two apart"""
    t = lambda a, g=False: torch.tensor(a, dtype=dtype, requires_grad=g)
    x = t(case["x"], True)
    gamma, beta = (t(case["gamma"], True), t(case["beta"], True)) if bn else (None, None)
    mean = x.mean(0)
    var = ((x * x).mean(0) - mean * mean).clamp_min(0) if uncentred else x.var(0, unbiased=False)      # tf.nn.moments
    if bn == "batch":
        m, invstd = mean, 1.0 / torch.sqrt(var + eps)
    elif bn == "moving":
        m, invstd = t(case["moving_mean"]), 1.0 / torch.sqrt(t(case["moving_var"]) + eps)
    if bn:
        xh = (x - m) * invstd
        z = xh * gamma + beta
    else:
        z = x * 1.0
    z.retain_grad()
    out = torch.relu(z) if activation == "relu" else torch.nn.functional.leaky_relu(z, 0.2) if activation == "leaky_relu" else z
    f64 = lambda a: a.detach().double().numpy()
    res = dict(out=f64(out), min_abs_z=float(z.detach().abs().min()))
    if bn:
        res.update(save_mean=f64(m), save_invstd=f64(invstd))
    if bn == "batch":
        # floors: the allowances per column that the float32 rounding of the MEAN alone accounts for.  save_mean is a float: it is off the true mean by up to
        # half a unit in its last place, |dm| <= eps32 / 2 |mean|; the subtraction x - mean rounds once more when the two are far apart: eps32 |mean| is
        # taken.  Every xhat of the column is then shifted by e = dm invstd, whatever the kernel does, so
        #   out        moves by  e |gamma|
        #   grad_gamma = sum dz xhat  by  e |sum dz|
        #   grad_x     = gamma invstd (dz - sum dz / N - xhat sum(dz xhat) / N)  by  gamma invstd e (|sum dz xhat| + max|xhat| |sum dz|) / N
        # and grad_beta = sum dz does not move at all.  With |mean| of the size of the spread these are below the 1e-4 contract; at |mean| / std = 1e4, or
        # at two rows that nearly coincide, they are what float32 leaves
        e = 2.0 ** -23 * np.abs(f64(m)) * f64(invstd)
        res["floors"] = dict(e=e, out=e * np.abs(case["gamma"].astype(np.float64)))
    res["moving_mean"] = case["moving_mean"].astype(np.float64) * momentum + f64(mean) * (1 - momentum)
    res["moving_var"] = case["moving_var"].astype(np.float64) * momentum + f64(var) * (1 - momentum)
    if backward:
        out.backward(t(case["go"]))
        res["grad_x"] = f64(x.grad)
        if bn == "batch":
            # the magnitudes of the terms of grad_x = gamma invstd (dz - sum dz / N - xhat sum(dz xhat) / N), per entry (close_columns' `terms`)
            N, dz, xhd = x.shape[0], z.grad, xh.detach()
            res["grad_x_terms"] = f64((gamma.detach() * invstd).abs() * (dz.abs() + dz.sum(0).abs() / N + xhd.abs() * (dz * xhd).sum(0).abs() / N))
        if bn == "batch":
            # what the float32 rounding of the MEAN alone accounts for (`floors`, below), backward part
            e, g_abs, xa = res["floors"]["e"], np.abs(case["gamma"].astype(np.float64)), f64(xh.abs().max(0).values)
            res["floors"]["grad_gamma"] = e * np.abs(f64(beta.grad))
            res["floors"]["grad_x"] = g_abs * f64(invstd) * e * (np.abs(f64(gamma.grad)) + xa * np.abs(f64(beta.grad))) / x.shape[0]
        if bn:
            res.update(grad_gamma=f64(gamma.grad), grad_beta=f64(beta.grad), beta_total=f64(z.grad.abs().sum(0)),
                       gamma_total=f64((z.grad * xh.detach()).abs().sum(0)))
    return res


def close_columns(got, ref, what="", bound=1e-4, floor=None, terms=None):
    """every entry within `bound` of ITS COLUMN's scale; floor (C,) or None: an absolute allowance per column added to the bound (the caller derives it).
    terms (rows, C) or None: the entry is a difference that CANCELS, and terms holds the sum of the magnitudes of what is subtracted; the contract measures an
    error against the array's own magnitude, which for such an entry is not |ref| (tests/pointwise_mlp_layers_oracle.close_sum says the same of a sum): two
    rows give grad_x = (dz_1 - dz_2) / 2 * eps / (var + eps), a thousandth of dz.  The expression is at most eight float operations on values no larger
    than `terms`, each rounding by at most 2^-24 of its result: where 2^-21 terms is larger than the column's bound it is the bound"""
    got, ref = np.atleast_2d(np.asarray(got, np.float64)), np.atleast_2d(np.asarray(ref, np.float64))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what + ": not finite"
    if ref.size == 0:
        return 0.0
    allowed = bound * np.maximum(np.abs(ref).max(0), 1e-30) * np.ones_like(ref)
    if terms is not None:
        allowed = np.maximum(allowed, 2.0 ** -21 * np.asarray(terms, np.float64))
    allowed = allowed + (0.0 if floor is None else np.asarray(floor, np.float64))
    ratio = float((np.abs(got - ref) / allowed).max())
    print("%s: worst error / bound %.3f" % (what, ratio))
    assert ratio <= 1.0, "%s: an entry is off by %.3f times its column's bound" % (what, ratio)
    return ratio


def assert_flip_free(ref, activation):
    U.assert_flip_free(ref, activation)


def check(res, ref, bn="batch", what=""):
    """out, grad_x (per column), grad_gamma / grad_beta (sums), and under batch statistics the moving statistics.  -> the worst error in units of its bound"""
    floors = ref.get("floors", {})
    worst = close_columns(res["out"], ref["out"], what + " out", floor=floors.get("out"))
    if "grad_x" in ref and "grad_x" in res:
        worst = max(worst, close_columns(res["grad_x"], ref["grad_x"], what + " grad_x", floor=floors.get("grad_x"), terms=ref.get("grad_x_terms")))
    for key, total in (("grad_gamma", "gamma_total"), ("grad_beta", "beta_total")):
        if key in ref and key in res:
            # (a sum: 1e-4 of the entry, or one fp32 unit of the total of ITS column's terms' magnitudes — close_sum, per column)
            g, r = np.asarray(res[key], np.float64), ref[key]
            allowed = np.maximum(1e-4 * np.abs(r), np.maximum(2.0 ** -23 * ref[total], 1e-34)) + floors.get(key, 0.0)
            ratio = float((np.abs(g - r) / allowed).max())
            assert np.isfinite(g).all() and ratio <= 1.0, "%s %s: worst %.3f of the bound" % (what, key, ratio)
            worst = max(worst, ratio)
    if bn == "batch" and "moving_mean" in res:
        U.close(res["moving_mean"], ref["moving_mean"], what + " moving mean")
        U.close(res["moving_var"], ref["moving_var"], what + " moving variance")
    return worst


def find_seed(shape=BASE, seeds=range(64)):
    for seed in seeds:
        case = make_case(*shape, seed)
        if all(reference(case, bn, "relu", backward=False)["min_abs_z"] >= 1e-5 for bn in BNS):
            return seed
    raise AssertionError("no flip-free seed")


if __name__ == "__main__":                                           # python -m tests.pool_bn_oracle: SEED
    print("SEED", find_seed())
