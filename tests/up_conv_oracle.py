"""TEST ORACLE: one decoder step of the segmentation head (tensorflow/models/heads/seg_head.py:63-67: nearest_upsample_block :13-28 = ind_closest_pool,
basic_operators.py:175-192; tf.concat; conv1d_1x1, basic_operators.py:195-241) restated in float64 torch in the reference's DIRECT form under autograd: append
a zero row to the coarse features, gather column 0 of the upsample table (an id outside [0, n1) reads the zero row), torch.cat with the skip features, then
the unary layer of tests/unary_layer_oracle.py (imported, not restated: its matmul, batch norm, activation, `close`, `close_sum` and `find_seed`).  It uses
nothing of the kernels' decomposition (csrc/up_conv.hip, cbl_up_conv_*): no product of the coarse rows before the gather, no split of the weights, no
segment sum.  TensorFlow itself is absent, so — as for the rest of a14 / a15 — this is a restatement of the graph code, not a recording of it.

out, y, grad_coarse, grad_skip and grad_W are held to `close`, grad_biases / grad_gamma / grad_beta to `close_sum` with the oracle's totals, the moving
statistics to `close`.  Gradient cases with relu or leaky_relu run on seeds where no pre-activation z lies within 1e-5 of zero (found on the CPU with
find_seed, `python -m tests.up_conv_oracle`; asserted again by every such case)."""
import numpy as np
import torch

from tests import unary_layer_oracle as U

close = U.close
close_sum = U.close_sum
find_seed = U.find_seed
flip_free = U.flip_free
assert_flip_free = U.assert_flip_free
ACTIVATIONS = U.ACTIVATIONS
BNS = U.BNS
#       n2, n1, c_up, c_skip, c_out, k: three row tiles of the fine layer (the last ragged), one of the coarse layer, ragged panels, two column tiles
BASE = (150, 40, 36, 36, 72, 3)
HUB, UNREFERENCED, HUB_ROWS = 7, 39, 131                             # the base table: coarse row 7 is the nearest of 131 fine rows, coarse row 39 of none
# the first seed at BASE on which no z of any (bn, bias) combination lies within 1e-5 of zero
SEED = 0
# the kernels' tiles are 64 rows x 64 columns over panels of 64 contraction steps: one below, at and one above each edge, in each of the five sizes
EDGES = ([(n2, 40, 36, 36, 72, 3) for n2 in (63, 64, 65)] + [(150, n1, 36, 36, 72, 3) for n1 in (63, 64, 65)] +
         [(150, 40, c, 36, 72, 3) for c in (63, 64, 65)] + [(150, 40, 36, c, 72, 3) for c in (63, 64, 65)] + [(150, 40, 36, 36, c, 3) for c in (63, 64, 65)])
# c_up = 6 with c_out = 13: W_skip starts 78 floats into the variable (no multiple of 4: its rows are never 16-byte aligned); c_skip = 5; k = 1; one fine row
ODD = [(150, 40, 6, 36, 13, 3), (150, 40, 36, 5, 72, 3), (150, 40, 36, 36, 72, 1), (1, 40, 36, 36, 72, 3)]
# each weight-gradient product runs over at most ceil(rows / 512) chunks of its own rows (n2 for W_skip, n1 for W_up), each a multiple of 64 rows: one,
# two and three chunks (the third ragged: 384 + 384 + 332) of each product
CHUNKS = [(512, 1100, 20, 20, 12, 2), (1024, 512, 20, 20, 12, 2), (1100, 1024, 20, 20, 12, 2)]
# one shape past every grid cap a launch of the two calls has, in three cases.  The first: 2050 tiles of 64 rows in BOTH layers against the row-tile
# kernels' cap of 2048 (coarse @ W_up, the forward product, grad_coarse, grad_skip) and more fine rows than the column sums' 4 * 512.  The second: 1024
# column groups make a trip of the elementwise passes 2 rows, so 2100 rows are 1050 trips against their cap of 1024 (the normalise and the dy pass), and
# 300 * 4096 elements of the segment sum are 4800 workgroups of its one-channel kernel against its cap of 4096.  The third: c_out = 256 takes the segment
# sum's float4 kernel at 4 coarse rows a workgroup, 4125 workgroups against its cap of 4096
CAPS = [(64 * 2048 + 70, 64 * 2048 + 66, 8, 8, 8, 2), (2100, 300, 8, 8, 4096, 1), (300, 16500, 4, 4, 256, 1)]
# several row tiles and weight-gradient chunks in both layers (what the mirror's bit-for-bit cases and its comparison with the composed entries run on),
# and the first seed on which it is flip-free under every (bn, bias)
MULTI, SEED_MULTI = (1100, 600, 36, 36, 72, 2), 46
# the two products at the coarse layer's rows split their contraction where their 64 x 64 tiles are at most half of 256 compute units and every split keeps at
# least 4 panels of 64 steps (ul_split_of, csrc/up_conv.hip).  coarse @ W_up: 8 panels in two splits; 7 panels: below the rule; 18 panels in four splits
# of 5, 5, 5 and 3 panels, the last one ragged (1100 = 17 * 64 + 12); 129 x 2 tiles: past the rule although the panels would do.  grad_coarse: 9 panels of
# c_out = 520 in splits of 5 and 4, the last ragged
SPLITS = [(150, 40, 512, 36, 72, 2), (150, 40, 448, 36, 72, 2), (150, 40, 1100, 36, 72, 2), (300, 8200, 512, 8, 72, 1), (150, 40, 36, 36, 520, 2)]
EXTREMES = [(200, 50, 2304, 1152, 576, 3), (20000, 5000, 144, 144, 72, 3)]     # the head's up_conv0 and up_conv3 at few rows


def table(rng, n2, n1, k, kind="random"):
    """the upsample table (n2, k) int32.  Only column 0 counts; the other columns hold other VALID ids, which must be ignored.
    random: about one id in sixteen is a shadow id (n1, n1 + 3 or -1); base: HUB is the nearest of HUB_ROWS rows, UNREFERENCED of none, six shadow ids;
    shadow: shadow ids only"""
    inds = rng.integers(0, n1, (n2, k)).astype(np.int32)
    first = rng.integers(0, n1, n2)
    if kind == "base":
        others = np.array([j for j in range(n1) if j not in (HUB, UNREFERENCED)])
        first = rng.choice(others, n2)
        rows = rng.permutation(n2)
        first[rows[:HUB_ROWS]] = HUB
        first[rows[HUB_ROWS:HUB_ROWS + 6]] = [n1, n1, -1, n1 + 3, n1, -1]
    elif kind == "shadow":
        first = rng.choice([n1, -1, n1 + 3], n2)
    elif n2 > 1:
        shadow = rng.random(n2) < 1.0 / 16
        first[shadow] = rng.choice([n1, -1, n1 + 3], int(shadow.sum()))
    inds[:, 0] = first
    if k > 1:                                                        # column 1 never equals column 0: reading the wrong column cannot go unnoticed
        inds[:, 1] = (np.where((first >= 0) & (first < n1), first, 0) + 1 + rng.integers(0, max(n1 - 1, 1), n2)) % n1
    return np.ascontiguousarray(inds)


def make_case(n2, n1, c_up, c_skip, c_out, k, seed, kind="random"):
    """coarse (n1, c_up), inds (n2, k), skip (n2, c_skip), W (c_up + c_skip, c_out) — the one TF variable —, biases, the batch-norm variables, grad_out `go`;
    and x (n2, c_up + c_skip), the concatenation the reference forms (a copy of float32 values: exact), for the imported layer"""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    c_in = c_up + c_skip
    case = dict(coarse=f32(rng.normal(size=(n1, c_up))), inds=table(rng, n2, n1, k, kind), skip=f32(rng.normal(size=(n2, c_skip))),
                W=f32(rng.normal(size=(c_in, c_out)) / np.sqrt(c_in)), biases=f32(rng.normal(0, 0.5, c_out)),
                gamma=f32(rng.uniform(0.5, 1.5, c_out)), beta=f32(rng.normal(0, 0.3, c_out)),
                moving_mean=f32(rng.normal(0, 0.5, c_out)), moving_var=f32(rng.uniform(0.5, 2.0, c_out)), go=f32(rng.normal(size=(n2, c_out))))
    case["x"] = direct_input(torch.tensor(case["coarse"]), case["inds"], torch.tensor(case["skip"])).numpy()
    return case


def row_ids(inds, n1):
    first = torch.tensor(np.asarray(inds)[:, 0], dtype=torch.int64)
    return torch.where((first >= 0) & (first < n1), first, torch.full_like(first, n1))


def direct_input(coarse, inds, skip):
    """seg_head.py:63-64: ind_closest_pool (a zero row appended, column 0 gathered), then tf.concat((upsampled, skip), axis=1)"""
    upsampled = torch.cat([coarse, torch.zeros_like(coarse[:1])])[row_ids(inds, coarse.shape[0])]
    return torch.cat([upsampled, skip], 1)


def reference(case, bn="batch", activation="relu", bias=True, momentum=0.98, eps=1e-3, backward=True):
    """float64 results: out, y, the updated moving statistics, min_abs_z; under grad_out = case['go'] grad_coarse, grad_skip, grad_W, grad_biases,
    grad_gamma, grad_beta and the totals of close_sum.  The layer is tests/unary_layer_oracle.reference on the concatenation; its gradient with respect to
    that concatenation goes back through torch.cat and the gather by autograd"""
    ref = U.reference(case, bn, activation, False, bias, momentum, eps, backward)
    if backward:
        coarse = torch.tensor(case["coarse"], dtype=torch.float64, requires_grad=True)
        skip = torch.tensor(case["skip"], dtype=torch.float64, requires_grad=True)
        direct_input(coarse, case["inds"], skip).backward(torch.tensor(ref.pop("grad_x")))
        ref.update(grad_coarse=coarse.grad.numpy(), grad_skip=skip.grad.numpy())
    return ref


def check(res, ref, bn="batch", what=""):
    U.check(res, ref, bn, what)
    for key in ("grad_coarse", "grad_skip"):
        if key in ref and key in res:
            close(res[key], ref[key], what + " " + key)


GRID = [(bn, False, b) for bn in BNS for b in (True, False)]          # (bn, shortcut, bias) as find_seed takes them: the head has no shortcut


def base_case():
    return make_case(*BASE, SEED, kind="base")


def multi_case():
    return make_case(*MULTI, SEED_MULTI)


if __name__ == "__main__":                                           # python -m tests.up_conv_oracle: SEED and SEED_MULTI
    print("SEED", find_seed(lambda s: make_case(*BASE, s, kind="base"), GRID))
    print("SEED_MULTI", find_seed(lambda s: make_case(*MULTI, s), GRID))
