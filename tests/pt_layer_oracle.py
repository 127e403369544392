"""TEST ORACLE: the Point Transformer layer behind its q / k / v projections (contrastboundary_amd/csrc/pt_layer.hip; the reference's
pytorch/model/blocks.py:34-44) restated in float64 torch, with autograd for the gradients, and the one driver that calls the six entry points
    cbl_pt_layer_forward / _forward_eval / _backward                 C = 32 | 64, K = 8 | 16
    cbl_pt_layer_wide_forward / _wide_backward / _wide_backward_csr  C = 128 | 256 | 512, K <= 64
through ctypes on the buffers of a backend (tests/attention_oracle.HostBackend, tests/test_gpu_attention.DeviceBackend), so that the host-emulated library
(tests/test_pt_layer_oracle_host.py) and the device (tests/test_gpu_pt_layer_oracle.py) run the same calls against the same oracle:
    p_r = xyz[idx] - xyz            p0 = p_r Wp^T + bp          p1 = ReLU(BN_p(p0))         pe = p1 W3C^T + b3C
    w2 = ReLU(BN_c(x_k[idx] - x_q + pe)) Wa^T + ba              a = softmax_K(ReLU(BN_g(w2)) Wb^T + bb)
    out[i, c] = sum_k (x_v[idx] + pe)[i, k, c] a[i, k, c % G]
The three BatchNorms get three different eps and momenta and buffers that start from random values and a count of 3, so that an index mix-up between them shows.
A gradient through a ReLU is discontinuous where the pre-activation is 0: `make_flip_free` moves every scene away from that (no float64 pre-activation of the
three stages within 1e-5 of zero), after which EVERY entry of every output is compared under the 1e-4 contract (attention_oracle.close) — nothing is excluded
and there is no norm-wise fallback."""
import ctypes

import numpy as np
import torch

from tests.attention_oracle import close, small, neighbours, transposed
from tests.host_emul.host_build import size_t_results

PARAMS = ["Wp", "bp", "gamma_p", "beta_p", "W3C", "b3C", "gamma_c", "beta_c", "Wa", "ba", "gamma_g", "beta_g", "Wb", "bb"]
FEATURES = ["x_q", "x_k", "x_v"]
SAVED = ["p_r", "p0", "p1", "w2", "a"]
EPS = 1e-5                                                             # the three equal eps of the older host tests (`reference`)
# BN_p, BN_c, BN_g.  The eps differ by 1e-2 and more: an eps moves invstd by eps / (2 var) of itself and the variances here are 1 to 3, so an entry that hands one
# BatchNorm another's eps is off by 15 and more times the 1e-4 bound — three eps around 1e-5 (1e-5, 3e-5, 2e-5 were tried) differ by 1e-5 of invstd, which no
# comparison at 1e-4 sees: with them the entries passed every check with eps3[1] and eps3[2] swapped
EPS3, MOMENTUM3 = (1e-5, 3e-2, 1e-2), (0.1, 0.2, 0.05)
COUNT0 = 3                                                             # num_batches_tracked before the forward pass
ZERO_GRADS = dict(bp="Wp", ba="Wa", bb="Wb")                           # exactly 0 in float64: a bias in front of a BatchNorm (bp, ba), a shift of all K logits of a softmax (bb)

# the scenes (n, K, C) of the device file; tests/test_pt_layer_oracle_host.py builds every one of them flip-free without a GPU
NARROW_EDGE = [(16, 16, 64), (17, 8, 64), (41, 8, 32), (67, 16, 32), (130, 16, 64)]
NARROW_CAPS = [(2100, 16, 64), (4200, 8, 32), (4200, 16, 64), (8300, 8, 64), (8300, 16, 32), (16500, 8, 32), (33000, 8, 64), (66000, 8, 32)]
NARROW_EVAL = NARROW_EDGE + [(2100, 16, 64), (8300, 16, 32)]
WIDE_EXTRA = (520, 16, 512)                                            # pw_logits<64> past 2048 x 256 elements
WIDE_FORWARD_ONLY = (5500, 16, 128)                                    # not flip-free: pw_p1 past 1024 x 256 elements


def wide_scenes():
    from tests.test_gpu_attention import CAPS, EDGE
    return [s for s in EDGE + CAPS if s[2] >= 128] + [WIDE_EXTRA]


_i, _f, _z = ctypes.c_int, ctypes.c_float, ctypes.c_size_t


# ---------------------------------------------------------------------------------------------------------------- scenes
def knn(xyz, K):
    d = ((xyz[:, None, :] - xyz[None, :, :]) ** 2).sum(-1)
    return np.argsort(d, axis=1, kind="stable")[:, :K].astype(np.int32)


def inputs(n, K, C, seed):
    """float32: coordinates, the three projections, the 14 parameters, the gradient of the output, and (drawn last) the three BatchNorms' buffers before the
    forward pass — run_mean<q> / run_var<q>, q = 0 (BN_p), 1 (BN_c), 2 (BN_g); an evaluation-mode call normalises with them"""
    rng = np.random.default_rng(seed)
    G = C // 8
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    t = dict(xyz=rng.uniform(0, 1, (n, 3)).astype(np.float32), x_q=f(n, C), x_k=f(n, C), x_v=f(n, C),
             Wp=f(3, 3) * 2, bp=f(3) * 0.1, gamma_p=rng.uniform(0.5, 1.5, 3).astype(np.float32), beta_p=f(3) * 0.2,
             W3C=f(C, 3) * 0.5, b3C=f(C) * 0.1, gamma_c=rng.uniform(0.5, 1.5, C).astype(np.float32), beta_c=f(C) * 0.2,
             Wa=f(G, C) * 0.3, ba=f(G) * 0.1, gamma_g=rng.uniform(0.5, 1.5, G).astype(np.float32), beta_g=f(G) * 0.2,
             Wb=f(G, G) * 0.6, bb=f(G) * 0.1, g_out=f(n, C))
    for q, d in enumerate((3, C, G)):
        t["run_mean%d" % q] = f(d) * 0.3
        t["run_var%d" % q] = rng.uniform(0.5, 2.0, d).astype(np.float32)
    return t


def make(n, K, C, seed):
    """`inputs` with the K nearest neighbours of its own cloud as t['idx'] (small n: the distance matrix is dense)"""
    t = inputs(n, K, C, seed)
    t["idx"] = knn(t["xyz"], K)
    return t


# ---------------------------------------------------------------------------------------------------------------- float64
def _tensors(t, grad):
    return {k: torch.tensor(t[k], dtype=torch.float64, requires_grad=grad and k != "xyz") for k in ["xyz"] + FEATURES + PARAMS}


def _layer(T, ti, eps3, stats=None):
    """the layer on float64 tensors.  stats = None: train-mode BatchNorms (batch statistics, biased variance); else ([mean] * 3, [var] * 3) to normalise with.
    -> dict of tensors: the outputs, the three pre-activations z_p (n K, 3) / z_c (n K, C) / z_g (n K, G) and the statistics used"""
    n, K = ti.shape
    C = T["x_q"].shape[1]
    G = C // 8
    mean, var, invstd = [], [], []

    def bn(x, q, g, b):
        m, v = (x.mean(0), x.var(0, unbiased=False)) if stats is None else (stats[0][q], stats[1][q])
        s = 1.0 / torch.sqrt(v + eps3[q])
        mean.append(m); var.append(v); invstd.append(s)
        return (x - m) * s * g + b

    p_r = T["xyz"][ti] - T["xyz"][:, None, :]
    p0 = p_r @ T["Wp"].T + T["bp"]
    z_p = bn(p0.reshape(n * K, 3), 0, T["gamma_p"], T["beta_p"])
    p1 = torch.relu(z_p).reshape(n, K, 3)
    pe = p1 @ T["W3C"].T + T["b3C"]
    w = T["x_k"][ti] - T["x_q"][:, None, :] + pe
    z_c = bn(w.reshape(n * K, C), 1, T["gamma_c"], T["beta_c"])
    w2 = torch.relu(z_c) @ T["Wa"].T + T["ba"]
    z_g = bn(w2, 2, T["gamma_g"], T["beta_g"])
    logits = (torch.relu(z_g) @ T["Wb"].T + T["bb"]).reshape(n, K, G)
    a = torch.softmax(logits, dim=1)
    out = ((T["x_v"][ti] + pe).view(n, K, 8, G) * a.unsqueeze(2)).sum(1).view(n, C)       # channel c takes weight c % G
    return dict(out=out, p_r=p_r, p0=p0, p1=p1, w2=w2.reshape(n, K, G), a=a, z_p=z_p, z_c=z_c, z_g=z_g, mean=mean, var=var, invstd=invstd)


def reference_layer(idx, t, eps3=EPS3, momentum3=MOMENTUM3, training=True):
    """float64 dict.  training: out, the saved tensors p_r / p0 / p1 / w2 / a, mean / var (biased) / invstd of the three BatchNorms, their run_mean / run_var
    (unbiased) / count after nn.BatchNorm1d's update of t's buffers, and `grads`: the 17 gradients under the loss sum(out * g_out).  Otherwise the evaluation-mode
    formula: the same outputs, normalised with t's buffers."""
    ti = torch.from_numpy(idx.astype(np.int64))
    T = _tensors(t, training)
    stats = None
    if not training:
        stats = [[torch.tensor(t["%s%d" % (nm, q)], dtype=torch.float64) for q in range(3)] for nm in ("run_mean", "run_var")]
    with torch.set_grad_enabled(training):
        r = _layer(T, ti, eps3, stats)
    res = {k: r[k].detach().numpy() for k in ["out"] + SAVED}
    if not training:
        return res
    (r["out"] * torch.tensor(t["g_out"], dtype=torch.float64)).sum().backward()
    rows = idx.size
    for k in ("mean", "var", "invstd"):
        res[k] = [v.detach().numpy() for v in r[k]]
    res["run_mean"] = [(1 - momentum3[q]) * t["run_mean%d" % q].astype(np.float64) + momentum3[q] * res["mean"][q] for q in range(3)]
    res["run_var"] = [(1 - momentum3[q]) * t["run_var%d" % q].astype(np.float64) + momentum3[q] * res["var"][q] * (rows / max(rows - 1, 1)) for q in range(3)]
    res["count"] = COUNT0 + 1
    res["grads"] = {k: T[k].grad.numpy() for k in FEATURES + PARAMS}
    return res


def reference(t, K, C):
    """the older host tests' form (tests/test_pt_layer_host.py, tests/test_pt_layer_wide_host.py, smoke()): the table is t['idx'], the three eps are EPS
    -> out, the 17 gradients, {p1, w2, a}, {mean: [3 tensors], var: [3 tensors]}"""
    r = reference_layer(t["idx"], t, eps3=(EPS, EPS, EPS))
    return r["out"], r["grads"], {k: r[k] for k in ("p1", "w2", "a")}, dict(mean=[torch.from_numpy(m) for m in r["mean"]], var=[torch.from_numpy(v) for v in r["var"]])


def near_zero(idx, t, eps3=EPS3, delta=1e-5):
    """where a float64 train-mode pre-activation lies within delta of zero -> (z_p: (n, K, 3) bool, z_c: (n, K, C) bool, z_g: (n, K, G) bool, the smallest |z|,
    and for the points with a near-zero z_g (points, channels): per point the channel of x_q that moves its first such z_g (i, k, g) most — among the channels
    whose ReLU is open at the pair (z_c[i, k, c] > 0; through a closed one x_q[i, c] does not reach w2[i, k]) the one with the largest |Wa[g, c]|)"""
    n, K = idx.shape
    with torch.no_grad():
        T = _tensors(t, False)
        r = _layer(T, torch.from_numpy(idx.astype(np.int64)), eps3)
        bad = [(r[k].abs() < delta).reshape(n, K, -1).numpy() for k in ("z_p", "z_c", "z_g")]
        low = min(float(r[k].abs().min()) for k in ("z_p", "z_c", "z_g"))
        pts, ks, gs = np.nonzero(bad[2])
        pts, first = np.unique(pts, return_index=True)
        open_c = r["z_c"].reshape(n, K, -1)[pts, ks[first]] > 0
        channels = (open_c * T["Wa"][gs[first]].abs()).argmax(1).numpy()
    return bad[0], bad[1], bad[2], low, (pts, channels)


SMALL_SCENE_PAIRS = 16384


def make_flip_free(idx, t, eps3=EPS3, delta=1e-5, max_rounds=12, max_share=0.03, seed=0):
    """moves the fp32 scene, in place, until no float64 pre-activation of the three ReLU(BatchNorm(.)) stages lies within `delta` of zero.
    A scene of more than SMALL_SCENE_PAIRS pairs moves POINTS (`idx` is given, so a coordinate does not change the table):
        z_p near zero at (i, .):      xyz[i] += U(2e-4, 4e-4)
        z_c near zero at (i, ., c):   x_q[i, c] += U(2e-4, 4e-4)
        z_g near zero at (i, .):      one channel of x_q[i] += U(2e-3, 4e-3): one that reaches the pair's w2 (near_zero); a random channel has a closed
                                      ReLU between itself and w2 half of the time and then moves nothing
    (whole x_q rows do not converge: they shift the batch statistics and create as many new near-zero activations as they remove).  The share of points this
    touches is about K C 2e-5 * (the density of z at 0, about 0.4): under 1 % at the narrow widths, 1.6 % at K C = 2048.  A scene of at most
    SMALL_SCENE_PAIRS pairs cannot pay per point — one point of 16 is 6 %, and K C = 8192 at the widest width means 6.5 % of the points — and need not:
    there a channel with a near-zero pre-activation gets U(2e-4, 4e-4) added to its BatchNorm's beta, which moves all n K pre-activations of the channel
    alike, of which n K 2e-5 0.4 <= 0.13 land within delta anew, so the rounds shrink geometrically and no point is touched.
    Asserts: no pre-activation within delta at the end, at most `max_rounds` rounds, at most `max_share` of the points touched.  This is no exclusion — every
    entry is still compared — it keeps the scene's distribution.  -> (points touched, rounds), also printed."""
    rng = np.random.default_rng(seed)
    n, K = idx.shape
    C = t["x_q"].shape[1]
    touched = np.zeros(n, bool)
    by_point = idx.size > SMALL_SCENE_PAIRS
    u = lambda lo, size: rng.uniform(lo, 2 * lo, size).astype(np.float32)
    for r in range(max_rounds + 1):
        bad_p, bad_c, bad_g, low, (g_points, g_channels) = near_zero(idx, t, eps3, delta)
        count = int(bad_p.sum() + bad_c.sum() + bad_g.sum())
        if count == 0:
            break
        assert r < max_rounds, "still %d pre-activations within %.0e of a ReLU's edge after %d rounds" % (count, delta, max_rounds)
        if by_point:
            pts = np.flatnonzero(bad_p.any((1, 2)))
            t["xyz"][pts] += u(2e-4, (pts.size, 3))
            touched[pts] = True
            pc = bad_c.any(1)                                          # (n, C)
            t["x_q"][pc] += u(2e-4, int(pc.sum()))
            touched |= pc.any(1)
            t["x_q"][g_points, g_channels] += u(2e-3, g_points.size)
            touched[g_points] = True
        else:
            for key, bad in (("beta_p", bad_p), ("beta_c", bad_c), ("beta_g", bad_g)):
                ch = np.flatnonzero(bad.any((0, 1)))
                t[key][ch] += u(2e-4, ch.size)
    assert low >= delta
    share = float(touched.sum()) / n
    print("scene (%d, %d, %d): make_flip_free took %d rounds and touched %d of %d points (%.2f %%)" % (n, K, C, r, int(touched.sum()), n, 100 * share))
    assert share <= max_share, "make_flip_free touched %.2f %% of the points" % (100 * share)
    return int(touched.sum()), r


def case(n, K, C, flip_free=True):
    """-> (idx, inputs, points touched, rounds) of the scene a shape is tested on: seeds n + K + C"""
    seed = n + K + C
    idx, t = neighbours(n, K, seed), inputs(n, K, C, seed + 1)
    touched, rounds = make_flip_free(idx, t, seed=seed + 2) if flip_free else (0, 0)
    return idx, t, touched, rounds


def tables(idx, seed):
    """the processing orders a scene runs with: none (targets in index order), and a random permutation; each with the transposed table built to match
    -> {name: (order or None, inv_start, inv_src)}"""
    order = np.random.default_rng(seed).permutation(idx.shape[0]).astype(np.int32)
    return {"index order": (None,) + transposed(idx, None), "ordered": (order,) + transposed(idx, order)}


# ---------------------------------------------------------------------------------------------------------------- the entries
class LayerEntries:
    """the six entries of pt_layer.hip on one backend.  Every output — the scatter form's d x_k / d x_v too, which the call zeroes itself — and the constants
    block are pre-filled with NaN, the workspace with 0xFF bytes (NaN as floats) and it has exactly cbl_pt_layer[_wide]_workspace_bytes bytes.  A call that is
    expected to return an error code (`expect`) is checked to have left every output and buffer as it was.  `shift`: the name of one buffer that starts one
    float past a 16-byte boundary; `short`: bytes the workspace lacks."""

    def __init__(self, lib, backend):
        self.L, self.B = lib, backend
        size_t_results(lib)

    def _arr3(self, bufs):
        return (ctypes.c_void_p * 3)(*[self.B.ptr(b).value for b in bufs])

    def _buffers(self, idx, t, wide, shift):
        (n, K), C = idx.shape, t["x_q"].shape[1]
        B, G = self.B, C // 8
        nan = lambda *s: np.full(s, np.nan, np.float32)
        k = {nm: B.put(t[nm], int(nm == shift)) for nm in ["xyz", "g_out"] + FEATURES + PARAMS}
        k["idx"] = B.put(idx, int(shift == "idx"))
        for nm, d in (("p_r", 3), ("p0", 3), ("p1", 3), ("w2", G), ("a", G)):
            k[nm] = B.put(nan(n, K, d), int(nm == shift))
        k["out"] = B.put(nan(n, C))
        k["consts"] = B.put(nan(getattr(self.L, "cbl_pt_layer_wide_consts_floats" if wide else "cbl_pt_layer_consts_floats")()))
        if wide:
            k["bnc"] = B.put(nan(2 * C))
        k["rm"] = [B.put(t["run_mean%d" % q]) for q in range(3)]
        k["rv"] = [B.put(t["run_var%d" % q]) for q in range(3)]
        k["nb"] = [B.fill((1,), COUNT0, np.int64) for q in range(3)]
        return k

    def _workspace(self, n, K, C, wide, short):
        nbytes = int(getattr(self.L, "cbl_pt_layer_wide_workspace_bytes" if wide else "cbl_pt_layer_workspace_bytes")(_i(n), _i(K), _i(C))) - short
        nbytes = max(nbytes, 0)
        return self.B.fill((nbytes,), 0xFF, np.uint8), _z(nbytes)

    def forward(self, idx, t, order=None, mode="train", expect=0, shift=None, short=0):
        """mode: 'train' / 'eval' (narrow), 'wide' (train; takes no order) -> (numpy outputs, the buffers a backward call needs), or None after an expected error"""
        (n, K), C = idx.shape, t["x_q"].shape[1]
        B, P, wide = self.B, self.B.ptr, mode == "wide"
        assert not (wide and order is not None)
        k = self._buffers(idx, t, wide, shift)
        dord = None if order is None else B.put(order)
        ws, wsn = self._workspace(n, K, C, wide, short)
        eps3, mom3 = (_f * 3)(*EPS3), (_f * 3)(*MOMENTUM3)
        args = [_i(n), _i(K), _i(C)] + [P(k[nm]) for nm in ["xyz"] + FEATURES] + [P(k["idx"])] + ([] if wide else [P(dord)]) + [P(k[nm]) for nm in PARAMS]
        args += [eps3] + ([] if mode == "eval" else [mom3]) + [self._arr3(k["rm"]), self._arr3(k["rv"])] + ([] if mode == "eval" else [self._arr3(k["nb"])])
        args += [P(k[nm]) for nm in SAVED + ["out", "consts"]] + ([P(k["bnc"])] if wide else []) + [P(ws), wsn, B.stream]
        name = dict(train="cbl_pt_layer_forward", eval="cbl_pt_layer_forward_eval", wide="cbl_pt_layer_wide_forward")[mode]
        rc = getattr(self.L, name)(*args)
        assert rc == expect, "%s returned %d, expected %d" % (name, rc, expect)
        got = {nm: B.get(k[nm]) for nm in SAVED + ["out"] + (["bnc"] if wide else [])}
        got.update(run_mean=[B.get(b) for b in k["rm"]], run_var=[B.get(b) for b in k["rv"]], count=[int(B.get(b)[0]) for b in k["nb"]])
        if expect:
            assert all(np.isnan(got[nm]).all() for nm in SAVED + ["out"] + (["bnc"] if wide else [])) and np.isnan(B.get(k["consts"])).all(), name + " wrote an output"
            _unchanged(got, t, name)
            return None
        return got, k

    def backward(self, idx, t, kept=None, table=None, form="narrow", expect=0, shift=None, short=0):
        """form: 'narrow' (table = (order or None, inv_start, inv_src)), 'wide scatter' (no table), 'wide csr' (table as narrow; None for the call without its
        tables).  kept: the buffers of the forward call; None (argument checks) = fresh ones  -> the 17 gradients as numpy arrays, or None after an expected error"""
        (n, K), C = idx.shape, t["x_q"].shape[1]
        B, P, wide = self.B, self.B.ptr, form != "narrow"
        k = kept if kept is not None else self._buffers(idx, t, wide, shift)
        assert kept is None or shift is None
        tab = [None, None, None] if table is None else [None if x is None else B.put(x) for x in table]
        ws, wsn = self._workspace(n, K, C, wide, short)
        g = {nm: B.put(np.full(t[nm].shape, np.nan, np.float32)) for nm in FEATURES + PARAMS}
        args = [_i(n), _i(K), _i(C)] + [P(k[nm]) for nm in FEATURES] + [P(k["idx"])]
        if form == "narrow":
            args += [P(x) for x in tab] + [P(k[nm]) for nm in ("gamma_p", "W3C", "b3C", "gamma_c", "Wa", "gamma_g", "Wb")]
        else:
            args += ([P(x) for x in tab] if form == "wide csr" else []) + [P(k[nm]) for nm in ("gamma_p", "W3C", "b3C", "gamma_c", "beta_c", "Wa", "gamma_g", "Wb")]
        args += [P(k[nm]) for nm in SAVED + ["consts"]] + ([P(k["bnc"])] if wide else []) + [P(k["g_out"])] + [P(g[nm]) for nm in FEATURES + PARAMS] + [P(ws), wsn, B.stream]
        name = {"narrow": "cbl_pt_layer_backward", "wide scatter": "cbl_pt_layer_wide_backward", "wide csr": "cbl_pt_layer_wide_backward_csr"}[form]
        rc = getattr(self.L, name)(*args)
        assert rc == expect, "%s returned %d, expected %d" % (name, rc, expect)
        got = {nm: B.get(v) for nm, v in g.items()}
        if expect:
            assert all(np.isnan(v).all() for v in got.values()), name + " wrote a gradient"
            return None
        return got


def _unchanged(got, t, what):
    """the three BatchNorms' buffers hold the bits they were given"""
    for q in range(3):
        assert np.array_equal(got["run_mean"][q].view(np.uint32), t["run_mean%d" % q].view(np.uint32)), "%s: running mean %d changed" % (what, q)
        assert np.array_equal(got["run_var"][q].view(np.uint32), t["run_var%d" % q].view(np.uint32)), "%s: running variance %d changed" % (what, q)
        assert got["count"][q] == COUNT0, "%s: num_batches_tracked %d changed" % (what, q)


# ---------------------------------------------------------------------------------------------------------------- the checks
BN_NAMES = ("BN_p", "BN_c", "BN_g")


def check_forward(got, ref, tag):
    """out, the five saved tensors, the three BatchNorms' buffers after the update; the wide entry's bnc_stats = BN_c's mean | invstd"""
    for k in ["out"] + SAVED:
        close(got[k], ref[k], "%s %s" % (tag, k))
    for q in range(3):
        close(got["run_mean"][q], ref["run_mean"][q], "%s running mean of %s" % (tag, BN_NAMES[q]))
        close(got["run_var"][q], ref["run_var"][q], "%s running variance of %s" % (tag, BN_NAMES[q]))
        assert got["count"][q] == ref["count"], (tag, q, got["count"])
    if "bnc" in got:
        C = ref["out"].shape[1]
        close(got["bnc"][:C], ref["mean"][1], tag + " bnc_stats mean")
        close(got["bnc"][C:], ref["invstd"][1], tag + " bnc_stats invstd")


def check_eval(got, ref, t, tag):
    for k in ("out", "a", "w2", "p1"):
        close(got[k], ref[k], "%s %s" % (tag, k))
    _unchanged(got, t, tag)


def check_backward(got, ref, tag, gathered):
    """the 17 gradients; gathered (narrow, wide csr): the row of d x_k / d x_v of the target nobody lists is exactly 0"""
    grads = ref["grads"]
    for k in FEATURES + PARAMS:
        if k in ZERO_GRADS:
            small(got[k], 1e-4 * float(np.abs(grads[ZERO_GRADS[k]]).max()), "%s grad %s" % (tag, k))
        else:
            close(got[k], grads[k], "%s grad %s" % (tag, k))
    if gathered:
        n = got["x_k"].shape[0]
        assert (got["x_k"][n - 1] == 0.0).all() and (got["x_v"][n - 1] == 0.0).all(), tag + ": the unlisted target's row of grad x_k / x_v is not exactly 0"


def check_narrow(E, idx, t, ref, tag, seed):
    """forward and backward of one narrow scene, without and with an order"""
    for name, table in tables(idx, seed).items():
        got, kept = E.forward(idx, t, table[0])
        check_forward(got, ref, "narrow forward %s %s:" % (tag, name))
        check_backward(E.backward(idx, t, kept, table), ref, "narrow backward %s %s:" % (tag, name), True)


def check_wide(E, idx, t, ref, tag, seed):
    """forward of one wide scene, then its scatter backward and its gather backward without and with an order"""
    got, kept = E.forward(idx, t, mode="wide")
    check_forward(got, ref, "wide forward %s:" % tag)
    check_backward(E.backward(idx, t, kept, None, "wide scatter"), ref, "wide backward %s scatter:" % tag, False)
    for name, table in tables(idx, seed).items():
        check_backward(E.backward(idx, t, kept, table, "wide csr"), ref, "wide backward %s csr, %s:" % (tag, name), True)


CBL_ERR_BAD_ARG, CBL_ERR_WORKSPACE, CBL_ERR_UNSUPPORTED = -1, -2, -3      # include/cbl_amd.h


def check_arguments(E, wide):
    """every refused call returns its code and leaves the NaN-filled outputs and the buffers untouched"""
    bad_arg, unsupported, workspace = CBL_ERR_BAD_ARG, CBL_ERR_UNSUPPORTED, CBL_ERR_WORKSPACE
    if not wide:
        idx, t, _, _ = case(17, 8, 64, flip_free=False)
        tab = tables(idx, 1)["ordered"]
        for shift in ("x_q", "w2", "idx"):
            E.forward(idx, t, tab[0], "train", expect=bad_arg, shift=shift)
            E.forward(idx, t, tab[0], "eval", expect=bad_arg, shift=shift)
            E.backward(idx, t, None, tab, "narrow", expect=bad_arg, shift=shift)
        E.forward(idx, t, None, "train", expect=workspace, short=1)
        E.forward(idx, t, None, "eval", expect=workspace, short=1)
        E.backward(idx, t, None, tab, "narrow", expect=workspace, short=1)
        for n, K, C in ((16, 12, 64), (16, 8, 48)):
            idx, t, _, _ = case(n, K, C, flip_free=False)
            tab = tables(idx, 1)["ordered"]
            E.forward(idx, t, None, "train", expect=unsupported)
            E.forward(idx, t, None, "eval", expect=unsupported)
            E.backward(idx, t, None, tab, "narrow", expect=unsupported)
    else:
        idx, t, _, _ = case(23, 16, 128, flip_free=False)
        tab = tables(idx, 1)["ordered"]
        E.forward(idx, t, None, "wide", expect=workspace, short=1)
        E.backward(idx, t, None, None, "wide scatter", expect=workspace, short=1)
        E.backward(idx, t, None, tab, "wide csr", expect=workspace, short=1)
        E.backward(idx, t, None, None, "wide csr", expect=bad_arg)
        E.backward(idx, t, None, (tab[0], tab[1], None), "wide csr", expect=bad_arg)
        for n, K, C in ((16, 65, 128), (16, 8, 96)):
            idx, t, _, _ = case(n, K, C, flip_free=False)
            tab = tables(idx, 1)["ordered"]
            E.forward(idx, t, None, "wide", expect=unsupported)
            E.backward(idx, t, None, None, "wide scatter", expect=unsupported)
            E.backward(idx, t, None, tab, "wide csr", expect=unsupported)
