"""TEST ORACLE: PosPool (the reference's tensorflow/models/local_aggregation_operators.py:15-250, before pool_bn / activation / output_conv) restated in float64
numpy from the float32 inputs — the output and, for a given grad_out, d / d features — the scenes it is tested on, and the one driver that calls the three C
entries (cbl_pospool_forward, cbl_pospool_backward, cbl_pospool_backward_csr) through ctypes on the buffers of a backend (host arrays in
tests/test_pospool_oracle_host.py, device tensors in tests/test_gpu_pospool_oracle.py), so both run the same calls against the same oracle.
    out[p, c] = reduce_k geo[p, k, c // shared] * f[idx[p, k], c]         geo: a position embedding with `mid` entries of rel = (s[idx] - q) / radius, each
    shared by C / mid consecutive channels; the shadow index n0 is a zero feature row at the point (0, 0, 0); reduce = sum, mean (divided by the count of
    idx < padding_num, padding_num = idx.max(), plus 1e-5) or max (-65535 added on shadow entries; the gradient shared equally by the entries that attain the
    maximum, exact equality in float64).
The oracle is written from the graph code, not from the kernels: it builds the (rows, K, mid) embedding tensor, repeats it over the shared channels and reduces,
in float64 throughout, `s - q` included.  Nothing here uses autograd; the written-out gradient is held to finite differences of the oracle's own forward by the
host test.

A scene is one blob inside the radius (|rel| <= 0.9 on every pair, so the sine argument stays under 16 turns), translated far from the origin, in which every
support is a plausible neighbour of every query, so the neighbour table is drawn, not searched.  `geometry` asserts on the float64 quantities alone:
    * trailing shadow indices on a fifth of the rows, one row all shadow, one row that lists one support K times, a hub listed by exactly HUB_PAIRS = 131 pairs
      (no multiple of the gather's 4-pair step), three supports nobody lists: row 0 and row n0 - 1, whose feature rows are inf (the kernels' clamped loads of
      shadow neighbours read row 0), and row n0 - 2.
    * scenes built for 'max' are flip-free: for every (p, c) the largest product and the largest DIFFERENT-VALUED product differ by at least 1e-3 of the
      largest |product| among the K of that (p, c).  Equal values come from a repeated index (the same bits in fp32 as well) and from the planted tie alone: two distinct
      supports whose features in one channel are exactly 0 while every other product of that (p, c) is negative.  Offending features are re-drawn; the share
      of (p, c) re-drawn is below 1 %.  A second planted row has trailing shadow entries and, in one channel, real products that are all negative: its maximum
      is a real value, not -65535.
    * input rounding is not the kernel's error: the oracle evaluated with rel rounded to fp32 before the embedding agrees with the oracle proper within 2e-5
      of the comparison scale of `close` (kept as sc.share).
    * padded=False: the no-padding twin — no entry equals n0, padding_num is the largest real index listed; one row lists it beside others and one row is made
      of it alone (divided by 1e-5: values 1e5 times its neighbours', which is why `close` scales per row).
`close` is the project's 1e-4 contract (README: floats within 1e-4) taken per row, for every embedding; nothing is excluded."""
import ctypes
import functools

import numpy as np

from tests.attention_oracle import HostBackend  # noqa: F401  (the host buffers of the driver; the device file brings its own backend)
from tests.host_emul.host_build import size_t_results
from tests.kpconv_oracle import OFFSET, bits, tables, transposed  # noqa: F401

EMBEDDINGS = ("one", "xyz", "distance", "exp_-d", "direction_exp_-d", "direction_d", "sin_cos", "two_order", "three_order")     # include/cbl_amd.h
REDUCTIONS = ("sum", "mean", "max")
OK, ERR_BAD_ARG, ERR_UNSUPPORTED = 0, -1, -3
POISON, TIE_A, TIE_B, HUB, REPEATED = 0, 1, 2, 3, 4                    # support rows with a part to play; random draws are from FIRST_FREE .. n0 - 3
FIRST_FREE = 5
HUB_PAIRS = 131
MARGIN = 1e-3                                                          # of the largest |product| among the K of a (p, c)
ROUNDING_SHARE = 2e-5
SHADOW_MAX = -65535.0
BLOCK = 4 << 20                                                        # float64 entries of one (rows, K, C) block: 32 MB each, a handful alive at once

_i, _f, _z = ctypes.c_int, ctypes.c_float, ctypes.c_size_t

# The shapes (n, n0, K, C, embedding), each run in 'sum', 'mean' and 'max', and per shape the kernels they take (csrc/pospool.hip).  Forward, 'sum' / 'mean',
# C % 4 == 0 and 16-byte aligned rows: pospool_fwd_v4<2, MODE> — MODE 1 'sin_cos' with C % 12 == 0, MODE 2 'xyz' with C % 12 == 0, MODE 0 otherwise; L = C / 4
# lanes per point (at most 256 float4 columns per launch), 256 / L points per workgroup.  Everything else of the forward ('max', C % 4 != 0, unaligned rows) and
# the scatter backward: pospool_kernel<BWD>, one wave per point, lane = channel, K <= 128 ids staged in LDS.  Gather backward ('sum' / 'mean', C % 4 == 0):
# pospool_inv_count_kernel + pospool_bwd_csr_kernel<MODE>, the same MODE / L rules over the targets, four pairs per step.
EDGE = [(331, 40, 1, 12, "sin_cos"),          # fwd_v4 MODE 1, L = 3 (85 points per workgroup, one idle thread); K = 1: the prefetch clamps at its first load
        (120, 48, 3, 12, "xyz"),              # MODE 2, odd K: the second of the two-at-a-time slots is past the row in the last step
        (170, 30, 2, 4, "one"),               # MODE 0, L = 1: 256 points per workgroup, one float4 per point
        (40, 60, 17, 72, "sin_cos"),          # L = 18: 14 points per workgroup, 4 idle threads; odd K
        (37, 50, 26, 9, "sin_cos"),           # the C == 9 form [sin cos](x, y, z) + rel: C % 4 != 0, pospool_kernel for every reduction; the gather refuses
        (30, 70, 65, 36, "sin_cos"),          # 'max' / scatter: the second pass of the `k = lane; k += 64` staging loop holds one neighbour
        (29, 90, 128, 36, "sin_cos"),         # K = PP_KMAX: the staging loop's second pass is full
        (41, 57, 16, 33, "distance"),         # C % 4 != 0: pospool_kernel, scatter backward; the gather refuses
        (45, 52, 9, 18, "direction_exp_-d"),  # mid 9 [dir, d, dir, d, d], shared 2; C % 4 != 0
        (45, 52, 9, 72, "direction_exp_-d"),  # mid 4 [dir, d], shared 18: MODE 0, L = 18
        (43, 66, 12, 64, "direction_d"),      # mid 4, shared 16: MODE 0, L = 16
        (39, 58, 20, 64, "exp_-d"),           # mid 1; 'max' over one wave of 64 channels
        (33, 61, 26, 72, "two_order"),        # mid 9, shared 8: a lane's four channels straddle two monomials
        (37, 50, 26, 9, "three_order"),       # the C == 9 form (second order only)
        (31, 64, 26, 144, "three_order"),     # mid 18, shared 8: the cubic monomials under translation; 'max' over three channel passes of a wave
        (70, 40, 5, 1032, "sin_cos"),         # C4 = 258: two column chunks of L = 129 (one point per workgroup, 127 idle threads), forward and gather
        (70, 40, 5, 1152, "sin_cos")]         # the network's widest: two chunks of L = 144
EXACT_RADIUS = {(37, 50, 26, 9, "sin_cos"): 0.09375}                   # 3 / 32, the same number in fp32 and float64; every other scene has radius 0.1
AT_THE_ORIGIN = (40, 60, 17, 72, "sin_cos")                            # the one EDGE scene that is also run untranslated
UNALIGNED = (44, 60, 16, 72, "sin_cos")                                # rows one float past a 16-byte boundary: the forward leaves fwd_v4 for pospool_kernel<false>
NO_PADDING = [(40, 60, 17, 72, "sin_cos"), (120, 48, 3, 12, "xyz")]    # their twins without any entry equal to n0, run in 'mean'
BAD_K = (30, 70, 129, 36, "sin_cos")                                   # K > PP_KMAX: CBL_ERR_BAD_ARG from every entry (no scene: the call is refused)
BAD_C = (40, 60, 17, 10, "sin_cos")                                    # 10 is neither 9 nor a multiple of 6: CBL_ERR_UNSUPPORTED
# CAPS: past the hard caps in the source.  (n, n0, K, C, embedding, reduction):
CAPS = [(8209, 300, 5, 516, "sin_cos", "mean"),     # fwd_v4: L = 129, one point per workgroup: 8209 trips > 8192 workgroups, vend = 8216 with holes in the last eighth
        (24611, 300, 4, 264, "xyz", "mean"),        # fwd_v4 MODE 2: L = 66, three points per workgroup: 8204 trips; the wrapper's gather case (98444 pairs)
        (2000, 4133, 9, 516, "sin_cos", "mean"),    # gather: one target per workgroup, 4133 trips > 2 x 2048: three passes of its loop, also over an order_dst
        (16421, 6007, 9, 36, "sin_cos", "max"),     # pospool_kernel: 16421 points > 4096 workgroups x 4 waves: a wave's LDS rows are reused; forward and scatter
                                                    # (6007 supports: a feature is listed by ~25 rows, so re-drawing one rarely makes a new near-tie)
        (16421, 6007, 9, 9, "sin_cos", "mean"),     # the same in the C == 9 form
        (1048583, 64, 1, 4, "one", "mean")]         # pospool_inv_count_kernel: the only shape past 4096 x 256 points; (n, 1, 4) float64 on the CPU side


# ---------------------------------------------------------------------------------------------------------------- float64
def mid_of(pe, C):
    """`mid` of (embedding, C) as the graph code sets it, or 0 where its reshape [n, K, mid, C / mid] cannot work"""
    if pe in ("one", "distance", "exp_-d"):
        return 1
    if pe == "xyz":
        return 3 if C % 3 == 0 else 0
    if pe in ("direction_exp_-d", "direction_d"):
        m = 9 if C <= 18 else 4
        return m if C % m == 0 else 0
    if pe == "sin_cos":
        return C if (C == 9 or C % 6 == 0) else 0
    if pe == "two_order":
        return 9 if C % 9 == 0 else 0
    if pe == "three_order":
        return 9 if C == 9 else (18 if C % 18 == 0 else 0)
    raise NotImplementedError(pe)


def embedding(rel, pe, C):
    """(m, K, 3) float64 normalised offsets -> (m, K, mid) float64"""
    x, y, z = rel[..., 0:1], rel[..., 1:2], rel[..., 2:3]
    dist = np.sqrt((rel * rel).sum(-1, keepdims=True))
    if pe == "one":
        return np.ones_like(dist)
    if pe == "xyz":
        return rel
    if pe == "distance":
        return dist
    if pe == "exp_-d":
        return np.exp(-dist)
    if pe in ("direction_exp_-d", "direction_d"):
        direction = rel / (dist + 1e-6)
        d = np.exp(-dist) if pe == "direction_exp_-d" else dist
        return np.concatenate([direction, d, direction, d, d] if C <= 18 else [direction, d], -1)
    if pe == "sin_cos":
        fd = 1 if C == 9 else C // 6
        dim_mat = np.power(1000.0, (1.0 / fd) * np.arange(fd, dtype=np.float64))
        div = (100.0 * rel)[..., None] / dim_mat                      # (m, K, 3, fd)
        emb = np.concatenate([np.sin(div), np.cos(div)], -1).reshape(rel.shape[:2] + (6 * fd,))
        return np.concatenate([emb, rel], -1) if C == 9 else emb
    if pe in ("two_order", "three_order"):
        second = [rel, x * y, x * z, y * z, x * x, y * y, z * z]
        if pe == "two_order" or C == 9:
            return np.concatenate(second, -1)
        return np.concatenate(second + [x ** 3, y ** 3, z ** 3, x * x * y, x * x * z, y * y * x, y * y * z, z * z * x, z * z * y], -1)
    raise NotImplementedError(pe)


def _blocks(sc):
    step = max(1, BLOCK // (sc.K * sc.C))
    return [slice(a, min(a + step, sc.n)) for a in range(0, sc.n, step)]


def _products(sc, pe, rows, round32=False):
    """float64, for the query rows `rows`: real (m, K) bool, ids (m, K) with 0 at shadow entries, gfull (m, K, C) the factor of every feature,
    prod (m, K, C) = gfull * gathered features (0 at shadow entries)"""
    ids = sc.idx[rows]
    real = ids < sc.n0
    ids = np.where(real, ids, 0)
    nb = np.where(real[..., None], sc.s.astype(np.float64)[ids], 0.0)                 # the shadow point is (0, 0, 0)
    rel = (nb - sc.q[rows].astype(np.float64)[:, None, :]) / float(sc.radius)
    if round32:
        rel = rel.astype(np.float32).astype(np.float64)
    geo = embedding(rel, pe, sc.C)
    mid = mid_of(pe, sc.C)
    assert mid > 0 and geo.shape[-1] == mid, (pe, sc.C, geo.shape)
    gfull = np.repeat(geo, sc.C // mid, axis=-1)                       # [mid, shared] row-major: channel c takes entry c // shared
    nf = np.where(real[..., None], np.asarray(sc.f, np.float64)[ids], 0.0)            # the shadow row is zeros: a select, never a product with row 0
    return real, ids, gfull, gfull * nf


def reference(sc, pe, reduction, round32=False):
    """-> out (n, C), grad_features (n0, C) in float64, the gradient under the loss sum(out * sc.go)"""
    assert pe in EMBEDDINGS and reduction in REDUCTIONS
    go = sc.go.astype(np.float64)
    out, gf = np.zeros((sc.n, sc.C)), np.zeros((sc.n0, sc.C))
    padding_num = int(sc.idx.max())
    for rows in _blocks(sc):
        real, ids, gfull, prod = _products(sc, pe, rows, round32)
        if reduction == "max":
            vals = prod + np.where(real, 0.0, SHADOW_MAX)[..., None]
            out[rows] = vals.max(1)
            attained = vals == out[rows][:, None, :]
            coef = attained / attained.sum(1, keepdims=True) * go[rows][:, None, :] * gfull
        else:
            nn = 1.0 if reduction == "sum" else ((sc.idx[rows] < padding_num).sum(-1).astype(np.float64) + 1e-5)[:, None]
            out[rows] = prod.sum(1) / nn
            coef = gfull * (go[rows] / nn)[:, None, :]
        t = ids[real]                                                  # the shadow row's gradient is dropped
        o = np.argsort(t, kind="stable")
        ts = t[o]
        if ts.size:
            first = np.flatnonzero(np.r_[True, ts[1:] != ts[:-1]])
            gf[ts[first]] += np.add.reduceat(coef[real][o], first, axis=0)
    return out, gf


def max_figures(sc, pe):
    """float64, per (p, c) over the K entries of the 'max' reduction: gap = largest value - largest different value (inf where all are equal), tied = more
    than one entry attains the maximum, big = the largest |product|, first / runner = the k of the largest and of the largest different value"""
    gap, tied, big, first, runner = [], [], [], [], []
    for rows in _blocks(sc):
        real, _, _, prod = _products(sc, pe, rows)
        vals = prod + np.where(real, 0.0, SHADOW_MAX)[..., None]
        top = vals.max(1, keepdims=True)
        below = np.where(vals < top, vals, -np.inf)
        gap.append(top[:, 0] - below.max(1))
        tied.append((vals == top).sum(1) > 1)
        big.append(np.abs(prod).max(1))
        first.append(vals.argmax(1))
        runner.append(below.argmax(1))
    return tuple(np.concatenate(a) for a in (gap, tied, big, first, runner))


# ---------------------------------------------------------------------------------------------------------------- the contract
def row_scale(ref):
    row = np.abs(ref).max(1)
    return np.maximum(np.maximum(row, np.median(row)), 1e-30)[:, None]


def worst(got, ref):
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    assert got.shape == ref.shape and ref.ndim == 2, (got.shape, ref.shape)
    assert np.isfinite(ref).all()
    return float((np.abs(got - ref) / row_scale(ref)).max()) if np.isfinite(got).all() else float("inf")


def close(got, ref, tag):
    """the project's contract (README: floats within 1e-4) per row: |got - ref| <= 1e-4 max(max|ref_row|, median over rows of max|ref_row|) for EVERY entry —
    a large row cannot excuse the others; prints and returns the worst ratio of an error to its row's scale"""
    ratio = worst(got, ref)
    print("%s: worst |got - ref| / row scale %.3e" % (tag, ratio))
    assert ratio <= 1e-4, "%s: an entry is off by %.3e of its row's scale (bound 1e-4)" % (tag, ratio)
    return ratio


# ---------------------------------------------------------------------------------------------------------------- scenes
class Scene:
    """float32 / int32 inputs of one shape: q (n, 3), s (n0, 3), idx (n, K), f (n0, C), go (n, C), radius; what the generator placed: rep_row, shadow_row
    (the all-max-index row of a twin), tie (row, channel) or None, neg (row, channel) or None, redrawn (share of (p, c)); and per reduction it was built for
    ref[reduction] = (out, grad_features) in float64 and share[reduction] = the rounded-input oracle's worst ratios against them"""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.tag = "(%d, %d, %d, %d, %s)%s%s%s" % (self.n, self.n0, self.K, self.C, self.pe, "" if self.translated else " at the origin",
                                                   "" if self.padded else " without padding", "" if self.radius == np.float32(0.1) else " radius %g" % self.radius)


def _clip(v, r):
    return v * np.minimum(1.0, r / np.linalg.norm(v, axis=1))[:, None]


@functools.lru_cache(maxsize=None)
def geometry(n, n0, K, C, pe, seed, translated=True, radius=0.1, padded=True, reductions=REDUCTIONS):
    """the scene of a shape and an embedding, every condition of the module's docstring asserted; flip-free where 'max' is among `reductions`"""
    assert n >= 24 and n0 >= 16 and 1 <= K <= 128 and n * K >= 2 * HUB_PAIRS + 4 * K and mid_of(pe, C) > 0
    rng = np.random.default_rng(seed)
    radius = np.float32(radius)
    R = float(radius)
    # queries within 0.3 radii of the blob's centre, supports within 0.6: every pair is inside the radius, |rel| <= 0.9
    ql, sl = _clip(rng.normal(size=(n, 3)) * 0.12 * R, 0.3 * R), _clip(rng.normal(size=(n0, 3)) * 0.3 * R, 0.6 * R)
    shift = np.array(OFFSET if translated else (0.0, 0.0, 0.0))
    q, s = (ql + shift).astype(np.float32), (sl + shift).astype(np.float32)

    near = np.arange(FIRST_FREE, n0 - 2)                              # n0 - 2 and n0 - 1 are listed by nobody
    idx = near[rng.integers(0, near.size, (n, K))].astype(np.int32)
    rep_row, shadow_row, listed_row, tie_row, neg_row = n // 3, n // 3 + 1, n // 3 + 2, n // 2, n // 2 + 1
    assert listed_row < tie_row
    last = int(near[-1])                                              # the twin's padding_num
    if padded:
        rows = rng.choice(n, n // 5, replace=False)                   # trailing shadow neighbours, as the radius search pads
        for i, npad in zip(rows, rng.integers(1, max(1, K // 3) + 1, rows.size)):
            idx[i, K - npad:] = n0
        idx[shadow_row] = n0
    else:
        idx[shadow_row] = last
        idx[listed_row, 0] = last
    idx[rep_row] = REPEATED
    tie = neg = None
    if K >= 2:
        idx[tie_row] = np.where(idx[tie_row] == n0, near[0], idx[tie_row])
        idx[tie_row, 0], idx[tie_row, 1] = TIE_A, TIE_B
        if padded:
            idx[neg_row] = near[rng.integers(0, near.size, K)]
            idx[neg_row, K - max(1, K // 3):] = n0
    pos = np.arange(n * K)
    flat = idx.reshape(-1)
    free = pos[(flat < n0) & ~np.isin(pos // K, [rep_row, shadow_row, listed_row, tie_row, neg_row])]
    flat[rng.choice(free, HUB_PAIRS, replace=False)] = HUB
    idx = np.ascontiguousarray(idx)

    f = rng.normal(size=(n0, C)).astype(np.float32)
    f[POISON] = f[n0 - 1] = np.inf
    sc = Scene(n=n, n0=n0, K=K, C=C, pe=pe, seed=seed, translated=translated, padded=padded, radius=radius, q=q, s=s, idx=idx, f=f,
               go=rng.normal(size=(n, C)).astype(np.float32), rep_row=rep_row, shadow_row=shadow_row, listed_row=listed_row, padding_num=int(idx.max()))

    # the two planted rows: signs of the features they list, in the channel where the smallest |factor| of the row is largest
    frozen = np.zeros((n0, C), bool)

    def plant(row, skip, avoid=-1):
        real, ids, gfull, _ = _products(sc, pe, slice(row, row + 1))
        ks = np.flatnonzero(real[0])[skip:]
        smallest = np.abs(gfull[0, ks]).min(0) if ks.size else np.ones(C)
        if avoid >= 0:
            smallest[avoid] = -1.0
        c = int(smallest.argmax())
        for k in ks:
            f[ids[0, k], c] = -np.sign(gfull[0, k, c]) * (0.5 + abs(f[ids[0, k], c]))
        frozen[ids[0, real[0]], c] = True
        return row, c

    if K >= 2:
        tie = plant(tie_row, 2)
        f[TIE_A, tie[1]] = f[TIE_B, tie[1]] = 0.0
        if padded:
            neg = plant(neg_row, 0, avoid=tie[1])
    sc.tie, sc.neg = tie, neg

    redrawn = np.zeros((n, C), bool)
    if "max" in reductions:
        for rounds in range(12):
            gap, tied, big, first, runner = max_figures(sc, pe)
            bad = gap < MARGIN * big
            if not bad.any():
                break
            assert rounds < 11, "%s: still %d (p, c) within the margin after 11 rounds" % (sc.tag, int(bad.sum()))
            redrawn |= bad
            p, c = np.nonzero(bad)
            j = idx[p, runner[p, c]]                                  # the runner-up's feature alone (a real entry: -65535 is never within the margin)
            j = np.where(frozen[np.minimum(j, n0 - 1), c], idx[p, first[p, c]], j)
            assert (j < n0).all()
            keep = f[frozen]
            f[j, c] = rng.normal(size=j.size).astype(np.float32)
            f[frozen] = keep
        sc.redrawn = float(redrawn.mean())
        assert sc.redrawn < 0.01, (sc.tag, sc.redrawn)
        assert not (gap < MARGIN * big).any()
        if tie:
            real, ids, _, prod = _products(sc, pe, slice(tie_row, tie_row + 1))
            v = prod[0, :, tie[1]]
            assert v[0] == 0.0 and v[1] == 0.0 and ids[0, 0] != ids[0, 1] and (v[2:][real[0, 2:]] < 0.0).all() and tied[tie], "the planted tie is not one"
        if neg:
            real, _, _, prod = _products(sc, pe, slice(neg_row, neg_row + 1))
            assert real[0].any() and not real[0].all() and (prod[0, real[0], neg[1]] < 0.0).all(), "the all-negative channel is not one"
    else:
        sc.redrawn = 0.0

    # the conditions on the final table
    count = np.bincount(idx.reshape(-1), minlength=n0 + 1)
    assert idx.min() >= 0 and idx.max() <= n0
    assert count[POISON] == 0 and count[n0 - 1] == 0 and count[n0 - 2] == 0 and count[HUB] == HUB_PAIRS and HUB_PAIRS % 4 != 0
    assert (idx[rep_row] == REPEATED).all() and count[REPEATED] == K
    assert np.isinf(f[POISON]).all() and np.isinf(f[n0 - 1]).all() and np.isfinite(np.delete(f, [POISON, n0 - 1], 0)).all()
    if K >= 2:
        assert count[TIE_A] == 1 and count[TIE_B] == 1
    if padded:
        assert sc.padding_num == n0 and (idx[shadow_row] == n0).all() and int((idx == n0).any(1).sum()) >= n // 5
        assert (np.diff((idx == n0).astype(int), axis=1) >= 0).all(), "shadow indices are not trailing"
    else:
        assert count[n0] == 0 and sc.padding_num == last and (idx[shadow_row] == last).all() and (idx[listed_row] == last).sum() >= 1 and \
            (idx[listed_row] != last).any()
    rel_max = 0.0
    for rows in _blocks(sc):
        real, ids, _, _ = _products(sc, "one", rows)
        d = (s.astype(np.float64)[ids] - q[rows].astype(np.float64)[:, None, :]) / R
        rel_max = max(rel_max, float(np.abs(d[real]).max()) if real.any() else 0.0)
    assert rel_max <= 0.91, (sc.tag, rel_max)

    # input rounding is not the kernel's error
    sc.ref, sc.share = {}, {}
    for reduction in reductions:
        sc.ref[reduction] = reference(sc, pe, reduction)
        rounded = reference(sc, pe, reduction, round32=True)
        sc.share[reduction] = tuple(worst(r32, r) for r32, r in zip(rounded, sc.ref[reduction]))
        assert max(sc.share[reduction]) <= ROUNDING_SHARE, (sc.tag, reduction, sc.share[reduction])
    print("scene %s: %d pairs, |rel| <= %.2f, %.2f %% of (p, c) re-drawn, rounded-input share %s" %
          (sc.tag, n * K, rel_max, 100 * sc.redrawn, ", ".join("%s %.1e / %.1e" % ((r,) + sc.share[r]) for r in reductions)))
    return sc


def case(n, n0, K, C, pe, translated=True, padded=True, reductions=REDUCTIONS, seed=None):
    """the scene a shape is tested on (seed: n + n0 + K + C unless given; the radius from EXACT_RADIUS or 0.1), built once per process"""
    return geometry(n, n0, K, C, pe, n + n0 + K + C if seed is None else seed, translated, EXACT_RADIUS.get((n, n0, K, C, pe), 0.1), padded, tuple(reductions))


def empty_support(n, K, C, pe):
    """n0 == 0: every entry is the shadow neighbour (no condition to assert, and no float64 to compute: zeros, or -65535 for 'max')"""
    rng = np.random.default_rng(n + K + C)
    return Scene(n=n, n0=0, K=K, C=C, pe=pe, seed=0, translated=True, padded=True, radius=np.float32(0.1), padding_num=0,
                 q=(rng.normal(size=(n, 3)) * 0.03 + np.array(OFFSET)).astype(np.float32), s=np.zeros((0, 3), np.float32),
                 idx=np.zeros((n, K), np.int32), f=np.zeros((0, C), np.float32), go=rng.normal(size=(n, C)).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- the entries
class Entries:
    """the three PosPool entries on one backend.  Outputs are pre-filled with NaN (zeros for the scatter entry, which accumulates); the gather entry's workspace
    has exactly cbl_pospool_backward_csr_workspace_bytes(n) bytes (`short` bytes fewer on request); padding_num is a one-int buffer holding idx.max().  `shift`:
    features and out (forward) / grad_out and grad_features (gather) start that many floats past a 16-byte boundary.  Every call returns (status, array)."""

    def __init__(self, lib, backend):
        self.L, self.B = lib, backend
        size_t_results(lib)

    def _head(self, sc):
        return [_i(sc.n), _i(sc.n0), _i(sc.K), _i(sc.C)]

    @staticmethod
    def _cfg(sc, pe, reduction):
        return _f(float(sc.radius)), _i(EMBEDDINGS.index(pe)), _i(REDUCTIONS.index(reduction))

    def forward(self, sc, pe, reduction, shift=0, null_support=False):
        """null_support: support_points and features are passed as null pointers (what torch gives for the empty tensors of n0 == 0)"""
        B = self.B
        P = (lambda buf: None if null_support and (buf is s or buf is f) else B.ptr(buf))
        q, s, idx, f, pad = B.put(sc.q), B.put(sc.s), B.put(sc.idx), B.put(sc.f, shift), B.put(np.array([sc.padding_num], np.int32))
        out = B.put(np.full((sc.n, sc.C), np.nan, np.float32), shift)
        rc = self.L.cbl_pospool_forward(*self._head(sc), P(q), P(s), P(idx), P(f), *self._cfg(sc, pe, reduction), P(pad), P(out), B.stream)
        return rc, B.get(out)

    def scatter(self, sc, pe, reduction):
        B, P = self.B, self.B.ptr
        q, s, idx, f, go, pad = B.put(sc.q), B.put(sc.s), B.put(sc.idx), B.put(sc.f), B.put(sc.go), B.put(np.array([sc.padding_num], np.int32))
        gf = B.put(np.zeros((sc.n0, sc.C), np.float32))               # (put: a buffer with an address also where n0 == 0)
        rc = self.L.cbl_pospool_backward(*self._head(sc), P(q), P(s), P(idx), P(f), *self._cfg(sc, pe, reduction), P(pad), P(go), P(gf), B.stream)
        return rc, B.get(gf)

    def gather(self, sc, pe, reduction, table, shift=0, short=0):
        """cbl_pospool_backward_csr over `table` = (order_dst or None, inv_start, inv_src): numpy arrays, or buffers that are already the backend's"""
        B, P = self.B, self.B.ptr
        q, s, idx, go, pad = B.put(sc.q), B.put(sc.s), B.put(sc.idx), B.put(sc.go, shift), B.put(np.array([sc.padding_num], np.int32))
        tab = [B.put(t) if isinstance(t, np.ndarray) else t for t in table]
        nbytes = self.L.cbl_pospool_backward_csr_workspace_bytes(_i(sc.n)) - short
        ws = B.fill((nbytes,), 0, np.uint8)
        gf = B.put(np.full((sc.n0, sc.C), np.nan, np.float32), shift)
        rc = self.L.cbl_pospool_backward_csr(*self._head(sc), P(q), P(s), P(idx), *self._cfg(sc, pe, reduction), P(pad), P(go), *[P(t) for t in tab], P(gf),
                                             P(ws), _z(nbytes), B.stream)
        return rc, B.get(gf)


# ---------------------------------------------------------------------------------------------------------------- the checks
def check_forward(E, sc, reduction, shift=0):
    tag = "%s %s%s forward" % (sc.tag, reduction, ", rows shifted by one float" if shift else "")
    rc, out = E.forward(sc, sc.pe, reduction, shift=shift)
    assert rc == OK, (tag, rc)
    ratio = close(out, sc.ref[reduction][0], tag)
    if reduction == "max" and sc.padded:
        assert (out[sc.shadow_row] == np.float32(SHADOW_MAX)).all(), tag + ": the all-shadow row"
        if sc.neg:
            assert SHADOW_MAX < sc.ref["max"][0][sc.neg] < 0.0 and out[sc.neg] < 0.0 and out[sc.neg] > -60000.0, tag + ": the all-negative channel"
    return ratio


def check_scatter(E, sc, reduction):
    tag = "%s %s scatter" % (sc.tag, reduction)
    rc, gf = E.scatter(sc, sc.pe, reduction)
    assert rc == OK, (tag, rc)
    ratio = close(gf, sc.ref[reduction][1], tag + " grad features")
    assert (gf[[POISON, sc.n0 - 2, sc.n0 - 1]] == 0.0).all(), tag + ": the row of a target nobody lists is not exactly 0"
    return ratio


def check_gather(E, sc, reduction, table, form, same_bits=None):
    """one table: values, exact zeros for the targets nobody lists (written over NaN), the same bits on a second run and as `same_bits` (the result over another
    form of the table: every form lists a target's pairs ascending, so the sums are taken in the same order).  'max' and C % 4 != 0: the entry must refuse.
    Then the refusals of a workspace one byte short and of gradients that are not 16-byte aligned.  -> (ratio, grad_features) or None"""
    tag = "%s %s gather, %s" % (sc.tag, reduction, form)
    if reduction == "max" or sc.C % 4:
        rc, _ = E.gather(sc, sc.pe, reduction, table)
        assert rc == ERR_UNSUPPORTED, (tag, rc)
        return None
    rc, gf = E.gather(sc, sc.pe, reduction, table)
    assert rc == OK, (tag, rc)
    ratio = close(gf, sc.ref[reduction][1], tag + " grad features")
    assert (gf[[POISON, sc.n0 - 2, sc.n0 - 1]] == 0.0).all(), tag + ": the row of a target nobody lists is not exactly 0"
    rc, again = E.gather(sc, sc.pe, reduction, table)
    assert rc == OK and np.array_equal(bits(again), bits(gf)), tag + ": a second run gives other bits"
    if same_bits is not None:
        assert np.array_equal(bits(same_bits), bits(gf)), tag + ": other bits than over the table in index order"
    rc, _ = E.gather(sc, sc.pe, reduction, table, short=1)
    assert rc == ERR_BAD_ARG, (tag, "workspace one byte short", rc)
    rc, _ = E.gather(sc, sc.pe, reduction, table, shift=1)
    assert rc == ERR_BAD_ARG, (tag, "shifted gradients", rc)
    return ratio, gf


def check_refusals(E):
    """K = 129 > PP_KMAX: CBL_ERR_BAD_ARG; 'sin_cos' at C = 10: CBL_ERR_UNSUPPORTED — from all three entries, before anything is launched"""
    for (n, n0, K, C, pe), want in ((BAD_K, ERR_BAD_ARG), (BAD_C, ERR_UNSUPPORTED)):
        rng = np.random.default_rng(K + C)
        idx = rng.integers(0, n0 + 1, (n, K)).astype(np.int32)
        sc = Scene(n=n, n0=n0, K=K, C=C, pe=pe, seed=0, translated=False, padded=True, radius=np.float32(0.1), padding_num=int(idx.max()),
                   q=rng.normal(size=(n, 3)).astype(np.float32) * 0.03, s=rng.normal(size=(n0, 3)).astype(np.float32) * 0.03, idx=idx,
                   f=rng.normal(size=(n0, C)).astype(np.float32), go=rng.normal(size=(n, C)).astype(np.float32))
        for reduction in REDUCTIONS:
            assert E.forward(sc, pe, reduction)[0] == want and E.scatter(sc, pe, reduction)[0] == want, (sc.tag, reduction)
            assert E.gather(sc, pe, reduction, (None,) + transposed(idx, n0))[0] == want, (sc.tag, reduction)


def check_empty_support(E, n=37):
    """n0 == 0, n > 0: status 0, zeros for 'sum' / 'mean' (0 / 1e-5), -65535 for 'max' — at widths the vector forward would take were n0 > 0, with
    buffers of no element and with null pointers in their place"""
    for K, C, pe in ((3, 12, "sin_cos"), (5, 1032, "sin_cos"), (4, 12, "xyz"), (2, 4, "one"), (6, 9, "sin_cos")):
        sc = empty_support(n, K, C, pe)
        for reduction in REDUCTIONS:
            for null_support in (False, True):
                rc, out = E.forward(sc, pe, reduction, null_support=null_support)
                assert rc == OK, (sc.tag, reduction, null_support, rc)
                assert (out == np.float32(SHADOW_MAX if reduction == "max" else 0.0)).all(), (sc.tag, reduction, out[:2])
            rc, gf = E.scatter(sc, pe, reduction)
            assert rc == OK and gf.shape == (0, C), (sc.tag, reduction, rc)
            rc, _ = E.gather(sc, pe, reduction, (None, np.zeros(1, np.int32), np.zeros(1, np.int32)))
            assert rc == (ERR_UNSUPPORTED if reduction == "max" or C % 4 else OK), (sc.tag, reduction, rc)


def check_max_ties(E, sc):
    """'max' through the forward and the scatter entry at the planted rows: the two zero-valued neighbours share the gradient of their (p, c) equally, as do the
    K entries of the repeated row; the all-shadow row passes no gradient (checked through the oracle's rows, which hold exactly these shares)"""
    assert sc.tie is not None and sc.padded
    out_ref, gf_ref = sc.ref["max"]
    row, c = sc.tie
    assert out_ref[row, c] == 0.0
    rc, out = E.forward(sc, sc.pe, "max")
    assert rc == OK and out[row, c] == 0.0, (sc.tag, out[row, c])
    rc, gf = E.scatter(sc, sc.pe, "max")
    assert rc == OK
    close(gf, gf_ref, sc.tag + " max scatter grad features")
    # TIE_A and TIE_B are listed by the tie row alone, at a product of 0 that is the maximum of channel c and of no other channel by accident
    _, _, gfull, _ = _products(sc, sc.pe, slice(row, row + 1))
    for k, j in ((0, TIE_A), (1, TIE_B)):
        want = 0.5 * float(sc.go[row, c]) * gfull[0, k, c]
        assert gf_ref[j, c] == want, "the oracle does not halve the gradient of the tie"
        assert abs(gf[j, c] - want) <= 1e-4 * max(abs(want), 1e-30), (sc.tag, j, gf[j, c], want)
    # the repeated row: K equal products per channel, each entry gets 1 / K of the gradient and all K land on the one support
    _, _, gfull, _ = _products(sc, sc.pe, slice(sc.rep_row, sc.rep_row + 1))
    want = sc.go[sc.rep_row].astype(np.float64) * gfull[0, 0]
    assert np.allclose(gf_ref[REPEATED], want, rtol=1e-12, atol=0) and np.allclose(gf[REPEATED], want, rtol=1e-4, atol=1e-4 * np.abs(want).max())
