"""TEST ORACLE: the ConvNet's unary layer conv1d_1x1 (tensorflow/models/basic_operators.py:195-241) restated in float64 torch in the reference's DIRECT form
under autograd — tf.matmul(features, w) (+ biases), batch norm over all rows (tf.layers.batch_normalization as basic_operators.batch_norm sets it up:
tf.nn.moments' biased variance, moving = moving * momentum + batch * (1 - momentum) with the biased variance), the bottleneck's shortcut added before the
activation (backbone/resnet.py:158-192), relu / leaky_relu(0.2) / none.  It uses nothing of the kernels (csrc/unary_layer.hip): no tiles, no partial
statistics, no hand-written batch-norm gradient.  TensorFlow itself is absent, so — as for the rest of a14 / a15 — this is a restatement of the graph code,
not a recording of it: parity is unpinned by execution.

The contract is the project's 1e-4 (`close`, tests/pointwise_mlp_oracle.py); grad_gamma, grad_beta and grad_biases are sums over the rows and are held to
`close_sum` (tests/pointwise_mlp_layers_oracle.py) with the total of their terms' magnitudes: under batch statistics grad_biases = sum dy cancels to zero in
exact arithmetic.  Gradient cases with relu or leaky_relu run on seeds where no pre-activation z lies within 1e-5 of zero (find_seed, on the CPU; the
precondition is asserted on the reference again by every such case)."""
import numpy as np
import torch

from tests import pointwise_mlp_layers_oracle as PL

close = PL.close
close_sum = PL.close_sum
ACTIVATIONS = {"none": 0, "relu": 1, "leaky_relu": 2}
BNS = ("batch", "moving", None)
BASE = (150, 36, 72)                                                  # rows, c_in, c_out: three row tiles (the last ragged), one ragged panel, two column tiles
# the first seed at BASE on which no z of any (bn, shortcut, bias) combination lies within 1e-5 of zero; the same for the case of column means near 8
SEED, SEED_MEAN_8 = 0, 0
# the kernels' tiles are 64 rows x 64 columns over panels of 64 contraction steps: one below, at and one above each edge; one row; c_in = 5 (the input conv:
# rows of 20 bytes, never 16-byte aligned); (150, 36, 13) is segmentation_pred's width
EDGES = [(63, 36, 72), (64, 36, 72), (65, 36, 72), (150, 63, 72), (150, 64, 72), (150, 65, 72), (150, 36, 63), (150, 36, 64), (150, 36, 65), (1, 36, 72),
         (150, 5, 72), (150, 36, 13)]
# grad_weights runs over at most ceil(rows / 512) chunks, each a multiple of 64 rows: one chunk, exactly two, three with a ragged last one (384 + 384 + 332)
CHUNKS = [(512, 20, 12), (1024, 20, 12), (1100, 20, 12)]
# one shape past every grid cap a launch has, in two cases.  The first: 2050 tiles of 64 rows against the row-tile kernels' cap of 2048 (forward, grad_x) and
# more rows than the column sums' 4 * 512 — but only 129 trips of the elementwise passes (2 column groups: 1024 rows a trip).  The second: 1024 column
# groups make a trip 2 rows, so 2100 rows are 1050 trips against the elementwise passes' cap of 1024 (the normalise and the dy pass)
CAPS = [(64 * 2048 + 70, 8, 8), (2100, 8, 4096)]
EXTREMES = [(200, 3456, 576), (100, 1152, 2304), (20000, 72, 72)]      # the head's up_conv0, the widest bottleneck conv, the first stage at many rows


def make_case(rows, c_in, c_out, seed, mean_8=False):
    """x, weights (c_in, c_out), biases, shortcut, the batch-norm variables and grad_out `go`; mean_8: features of mean 1 and weights with 8 / c_in added, so
    that y's columns have means near 8 and a standard deviation near 1"""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    case = dict(x=f32(rng.normal(size=(rows, c_in)) + (1.0 if mean_8 else 0.0)),
                W=f32(rng.normal(size=(c_in, c_out)) / np.sqrt(c_in) + (8.0 / c_in if mean_8 else 0.0)),
                biases=f32(rng.normal(0, 0.5, c_out)), shortcut=f32(rng.normal(size=(rows, c_out))),
                gamma=f32(rng.uniform(0.5, 1.5, c_out)), beta=f32(rng.normal(0, 0.3, c_out)),
                moving_mean=f32(rng.normal(0, 0.5, c_out)), moving_var=f32(rng.uniform(0.5, 2.0, c_out)), go=f32(rng.normal(size=(rows, c_out))))
    return case


def reference(case, bn="batch", activation="relu", shortcut=True, bias=True, momentum=0.98, eps=1e-3, backward=True):
    """float64 results: out, y; under grad_out = case['go'] the six gradients; the updated moving statistics; min_abs_z (the flip precondition) and the
    totals of the terms' magnitudes of the three column sums (close_sum)"""
    t = lambda a, g=False: torch.tensor(a, dtype=torch.float64, requires_grad=g)
    x, W = t(case["x"], True), t(case["W"], True)
    b = t(case["biases"], True) if bias else None
    sc = t(case["shortcut"], True) if shortcut else None
    gamma, beta = (t(case["gamma"], True), t(case["beta"], True)) if bn else (None, None)
    y = x @ W
    if bias:
        y = y + b
    y.retain_grad()
    mean, var = y.mean(0), y.var(0, unbiased=False)                   # tf.nn.moments
    if bn == "batch":
        xh = (y - mean) / torch.sqrt(var + eps)
    elif bn == "moving":
        xh = (y - t(case["moving_mean"])) / torch.sqrt(t(case["moving_var"]) + eps)
    else:
        xh = y
    z = xh * gamma + beta if bn else xh
    if shortcut:
        z = z + sc
    z.retain_grad()
    out = torch.relu(z) if activation == "relu" else torch.nn.functional.leaky_relu(z, 0.2) if activation == "leaky_relu" else z
    res = dict(out=out.detach().numpy(), y=y.detach().numpy(), min_abs_z=float(z.detach().abs().min()))
    res["moving_mean"] = case["moving_mean"].astype(np.float64) * momentum + mean.detach().numpy() * (1 - momentum)
    res["moving_var"] = case["moving_var"].astype(np.float64) * momentum + var.detach().numpy() * (1 - momentum)
    if backward:
        out.backward(t(case["go"]))
        res.update(grad_x=x.grad.numpy(), grad_W=W.grad.numpy(), biases_total=float(y.grad.abs().sum(0).max()))
        if bias:
            res["grad_biases"] = b.grad.numpy()
        if shortcut:
            res["grad_shortcut"] = sc.grad.numpy()
        if bn:
            res.update(grad_gamma=gamma.grad.numpy(), grad_beta=beta.grad.numpy(), beta_total=float(z.grad.abs().sum(0).max()),
                       gamma_total=float((z.grad * xh.detach()).abs().sum(0).max()))
    return res


def flip_free(ref, activation):
    return activation == "none" or ref["min_abs_z"] >= 1e-5


def assert_flip_free(ref, activation):
    """a relu flip between fp32 and float64 is not a kernel error: gradient cases with an activation run on seeds where none can occur"""
    if activation != "none":
        assert ref["min_abs_z"] >= 1e-5, "bad seed: a pre-activation within 1e-5 of zero (%.2e)" % ref["min_abs_z"]


def find_seed(make, configs, seeds=range(64)):
    """the first seed whose case make(seed) is flip-free under every (bn, shortcut, bias) of `configs` (z does not depend on the activation)"""
    for seed in seeds:
        case = make(seed)
        if all(reference(case, bn, "relu", sc, b, backward=False)["min_abs_z"] >= 1e-5 for bn, sc, b in configs):
            return seed
    raise AssertionError("no flip-free seed")


GRID = [(bn, sc, b) for bn in BNS for sc in (True, False) for b in (True, False)]


def base_case():
    return make_case(*BASE, SEED)


def check(res, ref, bn="batch", what=""):
    """out, y, every gradient present in both, and under batch statistics the moving statistics, within the 1e-4 contract"""
    close(res["out"], ref["out"], what + " out")
    if res.get("y") is not None:
        close(res["y"], ref["y"], what + " y")
    for key in ("grad_x", "grad_W", "grad_shortcut"):
        if key in ref and key in res:
            close(res[key], ref[key], what + " " + key)
    for key, total in (("grad_biases", "biases_total"), ("grad_gamma", "gamma_total"), ("grad_beta", "beta_total")):
        if key in ref and key in res:
            close_sum(res[key], ref[key], ref[total], what + " " + key)
    if bn == "batch" and "moving_mean" in res:
        close(res["moving_mean"], ref["moving_mean"], what + " moving mean")
        close(res["moving_var"], ref["moving_var"], what + " moving variance")


if __name__ == "__main__":                                           # python -m tests.unary_layer_oracle: SEED and SEED_MEAN_8
    print("SEED", find_seed(lambda s: make_case(*BASE, s), GRID))
    print("SEED_MEAN_8", find_seed(lambda s: make_case(*BASE, s, mean_8=True), [("batch", False, False), ("batch", True, True)]))
