"""TEST ORACLE: AdaptiveWeight with fc_num 2 and 3 (tensorflow/models/local_aggregation_operators.py:316-500; the layers :419-430: fc_0 .. fc_{fc_num-2} with the
network's activation, fc_{fc_num} without, every one of width M = mid_fdim, with bias, no batch norm), restated in float64 torch in the reference's DIRECT
form: gather the neighbourhoods, concatenate the blocks of `local_input_feature`, run the MLP per pair, softmax over the neighbours, reshape-multiply, reduce.
Geometry, first-layer weights, tolerances and option tables are those of tests/adaptive_weight_general_oracle.py; the fold of the first layer into per-point
terms that the kernels use (csrc/adaptive_weight_mlp.hip) is NOT used here.  TensorFlow itself is absent: a restatement of the graph code, not a recording.
Besides the results it returns the two flip figures of the project: min_abs_z, the smallest |pre-activation| of any hidden unit of any pair (a relu that
switches between fp32 and float64 is not a kernel error), and min_gap for 'max'."""
import numpy as np
import torch

from tests import adaptive_weight_general_oracle as G

MODES, SOFTMAX, REDUCTIONS, SOFTMAXES, close, RADIUS = G.MODES, G.SOFTMAX, G.REDUCTIONS, G.SOFTMAXES, G.close, G.RADIUS
ACTIVATIONS = {"relu": 1, "leaky_relu": 2}                           # any other string: the identity (basic_operators.py:285-289)
MIN_ABS_Z, MIN_GAP = 1e-5, 5e-5                                      # pointwise_mlp_oracle.assert_flip_free's thresholds


def make_case(n0, n, K, C, seed, mode, shared_channels=1, fc_num=2, activation="relu", last_scale=1.0, last_shift=0.0, **kw):
    """adaptive_weight_general_oracle.make_case plus the layers behind the first: weights ~ N(0, 1 / M) (M, M), biases ~ N(0, 0.3) (M) from
    default_rng(2000 + seed), all weights first and then all biases.  last_scale / last_shift: the last layer's weights times / bias plus (the stability case)"""
    case = G.make_case(n0, n, K, C, seed, mode, shared_channels, **kw)
    M = C // case["S"]
    rng = np.random.default_rng(2000 + seed)
    hw = [(rng.normal(size=(M, M)) / np.sqrt(M)).astype(np.float32) for _ in range(fc_num - 1)]
    hb = [rng.normal(0, 0.3, M).astype(np.float32) for _ in range(fc_num - 1)]
    hw[-1] = (hw[-1] * last_scale).astype(np.float32)
    hb[-1] = (hb[-1] + last_shift).astype(np.float32)
    case.update(hw=hw, hb=hb, activation=activation, fc_num=fc_num)
    return case


def act(x, activation):
    if activation == "relu":
        return torch.relu(x)
    if activation == "leaky_relu":
        return torch.nn.functional.leaky_relu(x, 0.2)
    return x


def direct(q, s, idx, f, W, b, hw, hb, radius, mode, S, softmax, reduction, activation):
    """-> out (n, C), the candidates of the maximum (n, K, C), the pre-activations of the hidden units [(n, K, M)]; float64 tensors"""
    n0, C = f.shape
    n, K = idx.shape
    idx = idx.long()
    sf = torch.cat([f, torch.zeros_like(f[:1])])
    sp = torch.cat([s, torch.zeros_like(s[:1])])
    fj = sf[idx]
    fi = sf[idx[:, :1]].expand(-1, K, -1)
    df = fj - fi
    dp = (sp[idx] - q[:, None]) / radius
    blocks = {"dp": [dp], "df": [df], "dp_df": [dp, df], "fj": [fj], "dp_fj": [dp, fj], "fi_df": [fi, df], "dp_fi_df": [dp, fi, df]}[mode]
    z = torch.cat(blocks, -1) @ W + b                                # fc_0
    pre = [z]
    for l in range(len(hw) - 1):                                     # fc_1 .. fc_{fc_num-2}
        z = act(z, activation) @ hw[l] + hb[l]
        pre.append(z)
    y = act(z, activation) @ hw[-1] + hb[-1]                         # fc_{fc_num}: no activation
    real = (idx < n0)
    kind = SOFTMAX[softmax]
    if kind == 2:
        w = torch.softmax(y, 1)
    elif kind == 1:
        m = real[..., None].expand_as(y)
        ninf = torch.full_like(y, -np.inf)
        mx = torch.where(m, y, ninf).amax(1, keepdim=True).detach()
        mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
        e = torch.exp(torch.where(m, y - mx, ninf))
        den = e.sum(1, keepdim=True)
        w = e / torch.where(den > 0, den, torch.ones_like(den))
    else:
        w = y
    a = (w[..., None] * fj.reshape(n, K, C // S, S)).reshape(n, K, C)
    if reduction == "max":
        cand = a + (~real).to(a.dtype)[..., None] * -65535.0
        return cand.amax(1), cand, pre
    out = a.sum(1)
    if reduction in ("mean", "avg"):
        out = out / ((idx < idx.max()).to(a.dtype).sum(-1, keepdim=True) + 1e-5)
    return out, a, pre


def reference(case, softmax, reduction, backward=True):
    """float64 results of one case: out, the gradients of f, W, b and of every hidden weight / bias under grad_out = case['go'], min_abs_z, min_gap"""
    t = lambda a, g=False: torch.tensor(a, dtype=torch.float64 if a.dtype.kind == "f" else torch.int64, requires_grad=g)
    f, W, b = t(case["f"], backward), t(case["W"], backward), t(case["b"], backward)
    hw, hb = [t(x, backward) for x in case["hw"]], [t(x, backward) for x in case["hb"]]
    out, cand, pre = direct(t(case["q"]), t(case["s"]), t(case["idx"]), f, W, b, hw, hb, case["radius"], case["mode"], case["S"], softmax, reduction,
                            case["activation"])
    res = dict(out=out.detach().numpy(), min_gap=np.inf, min_abs_z=min(float(z.detach().abs().min()) for z in pre))
    if backward:
        out.backward(t(case["go"]))
        res.update(grad_f=f.grad.numpy(), grad_W=W.grad.numpy(), grad_b=b.grad.numpy(), grad_hw=[x.grad.numpy() for x in hw],
                   grad_hb=[x.grad.numpy() for x in hb])
    if reduction == "max" and cand.shape[1] > 1:
        rows = (case["idx"] < case["f"].shape[0]).any(1)
        top = np.sort(cand.detach().numpy()[rows], 1)[:, -2:, :]
        if top.size:
            res["min_gap"] = float((top[:, 1] - top[:, 0]).min())
    return res


def flip_free(ref, case, reduction):
    return (case["activation"] not in ACTIVATIONS or ref["min_abs_z"] >= MIN_ABS_Z) and (reduction != "max" or ref["min_gap"] >= MIN_GAP)


def assert_flip_free(ref, case, reduction):
    """gradient cases with an activation or 'max' run on seeds where fp32 and float64 take the same branch everywhere"""
    if case["activation"] in ACTIVATIONS:
        assert ref["min_abs_z"] >= MIN_ABS_Z, "bad seed: a pre-activation within 1e-5 of 0 (%.2e)" % ref["min_abs_z"]
    if reduction == "max":
        assert ref["min_gap"] >= MIN_GAP, "bad seed: two candidates of a maximum within 5e-5 (%.2e)" % ref["min_gap"]


# ---------------------------------------------------------------- the cases both test files run
BASE = (96, 48, 10, 32)                                              # n0, n, K, C
SHARED = (1, 2)
FC_NUMS = (2, 3)
MEDIUM = (3000, 1500, 26, 72)
# the smallest seed of 0..19 at which the relu case of (fc_num, mode, S, softmax) at BASE meets min_abs_z >= 1e-5 and, under 'max', min_gap >= 5e-5
# (both asserted per case; found with seeds_table() below); 0 where not listed
_SEEDS = {(2, 'dp', 1, None): 2, (2, 'dp', 1, 'dense'): 4, (2, 'dp', 1, 'unmask'): 4, (2, 'dp', 2, 'dense'): 1, (2, 'dp', 2, 'unmask'): 6, (2, 'df', 1, None):
          3, (2, 'df', 1, 'dense'): 5, (2, 'df', 1, 'unmask'): 5, (2, 'df', 2, 'dense'): 2, (2, 'df', 2, 'unmask'): 2, (2, 'dp_df', 1, 'unmask'): 1, (2,
          'dp_df', 2, 'dense'): 1, (2, 'dp_df', 2, 'unmask'): 2, (2, 'fj', 1, None): 1, (2, 'fj', 1, 'dense'): 1, (2, 'fj', 1, 'unmask'): 1, (2, 'dp_fj', 1,
          'dense'): 1, (2, 'dp_fj', 1, 'unmask'): 1, (2, 'dp_fj', 2, 'dense'): 3, (2, 'dp_fj', 2, 'unmask'): 3, (2, 'fi_df', 1, 'dense'): 2, (2, 'fi_df', 1,
          'unmask'): 2, (2, 'fi_df', 2, None): 1, (2, 'fi_df', 2, 'dense'): 5, (2, 'fi_df', 2, 'unmask'): 5, (2, 'dp_fi_df', 1, 'dense'): 2, (2, 'dp_fi_df',
          1, 'unmask'): 3, (2, 'dp_fi_df', 2, None): 1, (2, 'dp_fi_df', 2, 'dense'): 2, (2, 'dp_fi_df', 2, 'unmask'): 2, (3, 'dp', 1, None): 2, (3, 'dp', 1,
          'dense'): 5, (3, 'dp', 1, 'unmask'): 18, (3, 'dp', 2, None): 1, (3, 'dp', 2, 'unmask'): 4, (3, 'dp_df', 1, None): 1, (3, 'dp_df', 1, 'dense'): 1,
          (3, 'dp_df', 1, 'unmask'): 1, (3, 'dp_df', 2, 'dense'): 1, (3, 'dp_df', 2, 'unmask'): 1, (3, 'fj', 1, None): 2, (3, 'fj', 1, 'dense'): 1, (3, 'fj',
          1, 'unmask'): 1, (3, 'dp_fj', 1, None): 2, (3, 'dp_fj', 1, 'dense'): 1, (3, 'dp_fj', 1, 'unmask'): 1, (3, 'dp_fj', 2, None): 1, (3, 'dp_fj', 2,
          'dense'): 7, (3, 'dp_fj', 2, 'unmask'): 12, (3, 'fi_df', 1, 'dense'): 1, (3, 'fi_df', 1, 'unmask'): 1}
# (n0, n, K, C, S): M = 16 in one tile; M = 20 padded to 32; M = 18; M = 36; M = 144 at K = 48; M = 72 of C = 576; K = 1, 16, 17, 33; K = 128 at M = 64;
# a single query; a last trip that is partly empty (50 queries of K = 10: trips of 6, 12 or 25 queries all end short)
SHAPES = [(96, 48, 10, 16, 1), (96, 48, 10, 20, 1), (96, 48, 10, 72, 4), (96, 48, 10, 36, 1), (160, 24, 48, 144, 1), (96, 8, 10, 576, 8), (96, 48, 1, 32, 1),
          (96, 48, 16, 32, 1), (96, 48, 17, 32, 1), (96, 48, 33, 32, 1), (160, 16, 128, 64, 1), (96, 1, 10, 32, 1), (96, 50, 10, 32, 1)]
HUB = (8, 48, 8, 32, 1)                                              # every target owns more pairs than one row tile


def base_case(fc_num, mode, S, softmax, activation="relu"):
    return make_case(*BASE, _SEEDS.get((fc_num, mode, S, softmax), 0), mode, S, fc_num, activation)


def flip_free_case(softmax, reductions, *args, **kw):
    """make_case(n0, n, K, C, seed, *args) at the smallest seed of 0..19 that is flip-free under every one of `reductions`"""
    for seed in range(20):
        case = make_case(*BASE, seed, *args, **kw)
        if all(flip_free(reference(case, softmax, r, backward=False), case, r) for r in reductions):
            return case
    raise AssertionError("no flip-free seed in 0..19")


def hub_case(seed, mode, fc_num, activation="none"):
    """HUB: the table of a (96, 48, 8) scene folded onto 8 support points (id % 8; shadow entries stay shadow), so every target owns about 40 pairs"""
    n0, n, K, C, S = HUB
    case = make_case(96, n, K, C, seed, mode, S, fc_num, activation, all_shadow_row=False)
    case["idx"] = np.where(case["idx"] < 96, case["idx"] % n0, n0).astype(np.int32)
    case["s"], case["f"] = np.ascontiguousarray(case["s"][:n0]), np.ascontiguousarray(case["f"][:n0])
    return case


def seeds_table():
    """recomputes _SEEDS (run by hand after a change of the generator): the smallest seed that is flip-free for 'sum' and for 'max' at once"""
    table = {}
    for fc_num in FC_NUMS:
        for mode in MODES:
            for S in SHARED:
                for softmax in SOFTMAXES:
                    for seed in range(20):
                        case = make_case(*BASE, seed, mode, S, fc_num)
                        if flip_free(reference(case, softmax, "max", backward=False), case, "max"):
                            break
                    else:
                        raise AssertionError("no flip-free seed in 0..19 for %r" % ((fc_num, mode, S, softmax),))
                    if seed:
                        table[(fc_num, mode, S, softmax)] = seed
    return table


def check(res, ref, case, softmax, what=""):
    """the 1e-4 contract (close: rtol 1e-4, atol 1e-4 max|ref|) on the output and every gradient `res` holds.  As in adaptive_weight_general_oracle.check, the
    rows of queries without a real neighbour are compared exactly.  Under a softmax the LAST layer's bias gradient is 0 by the shift invariance: the oracle's
    own value there is float64 rounding (asserted: below 1e-9 of its weight gradient) and the kernels' value must be exactly 0."""
    rows = (case["idx"] < case["f"].shape[0]).any(1)
    np.testing.assert_array_equal(res["out"][~rows], ref["out"][~rows], err_msg=what + " out of the queries without a real neighbour")
    if rows.any():
        close(res["out"][rows], ref["out"][rows], what + " out")
    if "grad_f" not in res:
        return
    close(res["grad_f"], ref["grad_f"], what + " grad features")
    close(res["grad_W"], ref["grad_W"], what + " grad fc_weight")
    # With the identity activation the whole MLP is linear, and under a softmax the shift invariance then reaches EVERY bias: their true gradients are 0 and
    # the oracle's values are rounding, which no relative bound can be taken from.  A bias is a weight row whose input is the constant 1, so the kernels'
    # value there is held to the absolute term of its own layer's weight gradient (1e-4 max|ref|), the oracle's to 1e-9 of it as for the last bias.
    linear = bool(SOFTMAX[softmax]) and case["activation"] not in ACTIVATIONS

    def zero_bias(got, ref_b, ref_w, name):
        assert np.abs(ref_b).max() <= 1e-9 * np.abs(ref_w).max()
        assert np.abs(np.asarray(got)).max() <= 1e-4 * np.abs(ref_w).max(), what + name
    if linear:
        zero_bias(res["grad_b"], ref["grad_b"], ref["grad_W"], " grad fc_bias (linear MLP under a softmax)")
    else:
        close(res["grad_b"], ref["grad_b"], what + " grad fc_bias")
    last = len(ref["grad_hw"]) - 1
    for l in range(last + 1):
        close(res["grad_hw"][l], ref["grad_hw"][l], what + " grad hidden weight %d" % l)
        if l == last and SOFTMAX[softmax]:
            assert np.abs(ref["grad_hb"][l]).max() <= 1e-9 * np.abs(ref["grad_hw"][l]).max()
            assert (np.asarray(res["grad_hb"][l]) == 0).all(), what + " grad of the last bias under a softmax"
        elif linear:
            zero_bias(res["grad_hb"][l], ref["grad_hb"][l], ref["grad_hw"][l], " grad hidden bias %d (linear MLP under a softmax)" % l)
        else:
            close(res["grad_hb"][l], ref["grad_hb"][l], what + " grad hidden bias %d" % l)
