"""TEST ORACLE: the ConvNet's scene-segmentation head (tensorflow/models/heads/seg_head.py:31-102) on a five-layer toy pyramid, in float64, as the composition
of the per-layer oracles: four decoder steps in the reference's direct form (tests/up_conv_oracle.py: gather, concat, unary layer), segmentation_head and
segmentation_pred (tests/unary_layer_oracle.py).  The forward pass feeds each layer's float64 output to the next; the backward pass hands each layer the
gradient of its output as its `go` and takes the gradient of its inputs back (the chain rule over the layers' own autograd) — no layer is restated here.
TensorFlow is absent: a restatement of the graph code, not a recording of it.

Every layer but segmentation_pred has a relu behind its batch norm: SEED is the first seed on which no pre-activation of any layer lies within 1e-5 of zero,
in training and in evaluation mode (`python -m tests.seg_head_oracle`, on the CPU; asserted again by the tests)."""
import numpy as np

from tests import unary_layer_oracle as U
from tests import up_conv_oracle as O

ROWS = (150, 70, 33, 17, 9)                                           # points of layers 0 .. 4
BASE_FDIM, NUM_CLASSES, MAX_NUM = 8, 13, 3
WIDTHS = tuple(2 ** (i + 1) * BASE_FDIM for i in range(5))            # F[i]: 16 .. 256
UP = ["up_conv%d" % s for s in range(4)]
LAYERS = UP + ["segmentation_head", "segmentation_pred"]
SEED = 0
BN_NAMES = (("gamma", "gamma"), ("beta", "beta"), ("moving_mean", "moving_mean"), ("moving_var", "moving_variance"))


def shapes():
    """layer -> (c_in, c_out)"""
    s = {}
    for step in range(4):
        out = 2 ** (3 - step) * BASE_FDIM
        s[UP[step]] = ((WIDTHS[4] if step == 0 else 2 * out) + 2 * out, out)
    s["segmentation_head"] = (BASE_FDIM, BASE_FDIM)
    s["segmentation_pred"] = (BASE_FDIM, NUM_CLASSES)
    return s


def make_case(seed):
    """F[i] (ROWS[i], WIDTHS[i]); upsamples[i] (ROWS[i - 1], MAX_NUM) for i = 1 .. 4 (upsamples[0] is never read), about one first id in sixteen a shadow
    id; per layer the variables under their state_dict names; the cotangent of the logits"""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    case = dict(F=[f32(rng.normal(size=(r, w))) for r, w in zip(ROWS, WIDTHS)],
                upsamples=[np.zeros((0, MAX_NUM), np.int32)] + [O.table(rng, ROWS[i - 1], ROWS[i], MAX_NUM) for i in range(1, 5)],
                go=f32(rng.normal(size=(ROWS[0], NUM_CLASSES))), params={})
    for layer, (c_in, c_out) in shapes().items():
        p = dict(weights=f32(rng.normal(size=(c_in, c_out)) / np.sqrt(c_in)))
        if layer == "segmentation_pred":
            p["biases"] = f32(rng.normal(0, 0.5, c_out))
        else:
            p.update(gamma=f32(rng.uniform(0.5, 1.5, c_out)), beta=f32(rng.normal(0, 0.3, c_out)), moving_mean=f32(rng.normal(0, 0.5, c_out)),
                     moving_variance=f32(rng.uniform(0.5, 2.0, c_out)))
        case["params"][layer] = p
    return case


def _layer_case(p, **inputs):
    c = dict(W=p["weights"], **inputs)
    if "biases" in p:
        c["biases"] = p["biases"]
    for key, name in BN_NAMES:
        if name in p:
            c[key] = p[name]
    if "gamma" not in p:                                             # (the layer oracle reports moving statistics whatever the mode: placeholders)
        c["moving_mean"] = c["moving_var"] = np.zeros(p["weights"].shape[1], np.float32)
    return c


def reference(case, training=True, backward=True):
    """-> dict(F_up (finest first), features, logits; min_abs_z over all relu layers; per layer moving_mean / moving_variance after the step (training);
    under the cotangent case['go'] on the logits: grad_F[i] and per layer the gradient of every parameter, with the totals close_sum wants)"""
    bn = "batch" if training else "moving"
    F, ups, params = case["F"], case["upsamples"], case["params"]
    # float64 activations travel between the layers as float64 arrays: the per-layer oracles convert their inputs with dtype=float64, which keeps them
    cases, outs, features, min_z = {}, {}, F[4].astype(np.float64), np.inf
    for step, layer in enumerate(UP):
        c = _layer_case(params[layer], coarse=features, inds=ups[4 - step], skip=F[3 - step])
        c["x"] = np.concatenate([np.concatenate([features, np.zeros_like(features[:1])])[O.row_ids(c["inds"], features.shape[0]).numpy()],
                                 F[3 - step].astype(np.float64)], 1)          # seg_head.py:63-64, as up_conv_oracle.direct_input forms it
        cases[layer] = c
        outs[layer] = O.reference(c, bn, "relu", False, backward=False)
        features = outs[layer]["out"]
        min_z = min(min_z, outs[layer]["min_abs_z"])
    F_up = [outs[layer]["out"] for layer in reversed(UP)]
    cases["segmentation_head"] = _layer_case(params["segmentation_head"], x=features)
    outs["segmentation_head"] = U.reference(cases["segmentation_head"], bn, "relu", False, False, backward=False)
    min_z = min(min_z, outs["segmentation_head"]["min_abs_z"])
    head = outs["segmentation_head"]["out"]
    cases["segmentation_pred"] = _layer_case(params["segmentation_pred"], x=head)
    outs["segmentation_pred"] = U.reference(cases["segmentation_pred"], None, "none", False, True, backward=False)
    res = dict(F_up=F_up, features=head, logits=outs["segmentation_pred"]["out"], min_abs_z=min_z, moving={}, grads={}, totals={})
    if training:
        res["moving"] = {layer: dict(moving_mean=outs[layer]["moving_mean"], moving_variance=outs[layer]["moving_var"]) for layer in LAYERS[:-1]}
    if not backward:
        return res

    def grads_of(layer, r, has_bn):
        res["grads"][layer] = dict(weights=r["grad_W"])
        res["totals"][layer] = {}
        if "grad_biases" in r:
            res["grads"][layer]["biases"] = r["grad_biases"]
            res["totals"][layer]["biases"] = r["biases_total"]
        if has_bn:
            res["grads"][layer].update(gamma=r["grad_gamma"], beta=r["grad_beta"])
            res["totals"][layer].update(gamma=r["gamma_total"], beta=r["beta_total"])

    r = U.reference(dict(cases["segmentation_pred"], go=case["go"]), None, "none", False, True)
    grads_of("segmentation_pred", r, False)
    r = U.reference(dict(cases["segmentation_head"], go=r["grad_x"]), bn, "relu", False, False)
    grads_of("segmentation_head", r, True)
    go, grad_F = r["grad_x"], [None] * 5
    for step in (3, 2, 1, 0):
        r = O.reference(dict(cases[UP[step]], go=go), bn, "relu", False)
        grads_of(UP[step], r, True)
        grad_F[3 - step] = r["grad_skip"]
        go = r["grad_coarse"]
    grad_F[4] = go
    res["grad_F"] = grad_F
    return res


def flip_free(seed):
    case = make_case(seed)
    return all(reference(case, training, backward=False)["min_abs_z"] >= 1e-5 for training in (True, False))


if __name__ == "__main__":                                           # python -m tests.seg_head_oracle: SEED
    print("SEED", next(s for s in range(64) if flip_free(s)))
