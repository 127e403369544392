"""TEST ORACLE: the C-wide passes of the Point Transformer layer (contrastboundary_amd/csrc/attention.hip) restated in float64 torch, with autograd for the
gradients, and the one driver that calls the ten entry points through ctypes on the buffers of a backend (host arrays here, device tensors in
tests/test_gpu_attention.py), so that the host-emulated library (tests/test_attention_oracle_host.py) and the device run the same calls against the same oracle:
    attn_w2   w2 = Linear(C, G)(ReLU(BN_C(x_k[idx] - x_q + p1 @ W3C^T + b3C)))      train-mode batch statistics, or supplied ones
    attn_agg  out = sum_k (x_v[idx] + p1 @ W3C^T + b3C) * w[..., c % G]            w = the weights, or the softmax of the logits over the K neighbours
A gradient through a ReLU is discontinuous where the pre-activation is 0, and fp32 and float64 may stand on different sides of it: `make_flip_free` moves every
scene away from that (no pre-activation within 1e-5 of zero, the precondition of tests/pointwise_mlp_oracle.assert_flip_free), after which EVERY entry of every
output is compared (`close`: 1e-4 relative, 1e-4 of the largest entry absolute) — nothing is excluded and there is no norm-wise fallback."""
import ctypes

import numpy as np
import torch

from tests.host_emul.host_build import size_t_results

EPS, MOMENTUM = 1e-5, 0.1
HUB, REPEATED = 2, 7                                                   # the unlisted target is n - 1, the repeated row n // 3
COUNT0 = 3                                                             # num_batches_tracked before the forward pass

_i, _f, _z = ctypes.c_int, ctypes.c_float, ctypes.c_size_t


# ---------------------------------------------------------------------------------------------------------------- scenes
def neighbours(n, K, seed):
    """(n, K) int32: self in column 0, random elsewhere; target n - 1 listed by nobody, target 2 by more than 3 K pairs (a count that is no multiple of 4, the
    gathers' unroll), row n // 3 lists target 7 K times.  The hub / the repeated row are left out where the table is too small to hold them."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n - 1, (n, K)).astype(np.int32)             # n - 1 never drawn
    idx[:n - 1, 0] = np.arange(n - 1)
    rep = n // 3 if n > REPEATED + 1 else -1
    if rep >= 0:
        idx[rep] = REPEATED
    flat = idx.reshape(-1)
    pos = np.arange(n * K)
    free = pos[(flat != HUB) & (pos // K != rep) & (pos % K != 0)]
    have = int((flat == HUB).sum())
    extra = max(3 * K + 1 - have, 0)
    extra += (have + extra) % 4 == 0
    hub = n > HUB + 1 and extra <= free.size
    if hub:
        flat[rng.choice(free, extra, replace=False)] = HUB
    count = np.bincount(flat, minlength=n)
    assert count[n - 1] == 0 and (np.delete(idx[:, 0], [rep % n, n - 1]) == np.delete(np.arange(n), [rep % n, n - 1])).all()
    assert not hub or (count[HUB] > 3 * K and count[HUB] % 4 != 0)
    assert rep < 0 or (idx[rep] == REPEATED).all()
    return idx


def transposed(idx, order):
    """the transposed table in numpy (independent of neighbor_transpose.hip): segment r of inv_src lists, ascending, the flat pairs p = i * K + k with
    idx[p] == (order[r] if an order is given else r)"""
    n = idx.shape[0]
    flat = idx.reshape(-1)
    by_target = np.argsort(flat, kind="stable").astype(np.int32)
    deg = np.bincount(flat, minlength=n)
    first = np.concatenate([[0], np.cumsum(deg)])
    if order is None:
        return first.astype(np.int32), by_target
    inv_start = np.concatenate([[0], np.cumsum(deg[order])]).astype(np.int32)
    inv_src = np.concatenate([by_target[first[j]:first[j + 1]] for j in order]).astype(np.int32)
    return inv_start, inv_src


def scene(n, K, C, seed):
    """float32 inputs of both passes, the distributions of tests/test_attention_host.scene; the softmax logits are twice as wide and one point's logits
    carry +-50 on alternating neighbours (without the subtraction of the maximum exp overflows; float64 torch.softmax is the truth).  `weights` are the
    plain weights of the pass without softmax; run_* the BatchNorm buffers before the forward pass; eval_* the statistics an evaluation-mode call is given."""
    rng = np.random.default_rng(seed)
    G = C // 8
    a = dict(x_q=rng.normal(size=(n, C)), x_k=rng.normal(size=(n, C)), x_v=rng.normal(size=(n, C)), p1=np.abs(rng.normal(size=(n, K, 3))),
             W3C=rng.normal(size=(C, 3)) * 0.5, b3C=rng.normal(size=C) * 0.1, gamma=rng.uniform(0.5, 1.5, C), beta=rng.normal(size=C) * 0.1,
             Wa=rng.normal(size=(G, C)) / np.sqrt(C), ba=rng.normal(size=G) * 0.1, weights=rng.normal(size=(n, K, G)), logits=2.0 * rng.normal(size=(n, K, G)),
             g_w2=rng.normal(size=(n, K, G)), g_out=rng.normal(size=(n, C)), run_mean=rng.normal(size=C) * 0.1, run_var=rng.uniform(0.5, 2.0, C),
             eval_mean=rng.normal(size=C) * 0.3, eval_invstd=rng.uniform(0.5, 1.5, C))
    a["logits"][n // 2, 0::2] += 50.0
    a["logits"][n // 2, 1::2] -= 50.0
    return {k: np.ascontiguousarray(v, np.float32) for k, v in a.items()}


# ---------------------------------------------------------------------------------------------------------------- float64
def _t(a, keys, grad):
    return {k: torch.tensor(a[k], dtype=torch.float64, requires_grad=grad) for k in keys}


def _pre_activation(ti, t, eps, stats=None):
    C = t["x_q"].shape[1]
    pre = t["x_k"][ti] - t["x_q"][:, None, :] + (t["p1"] @ t["W3C"].T + t["b3C"])
    if stats is None:
        flat = pre.reshape(-1, C)
        mean, var = flat.mean(0), flat.var(0, unbiased=False)
        invstd = 1.0 / torch.sqrt(var + eps)
    else:
        (mean, invstd), var = stats, None
    return (pre - mean) * invstd * t["gamma"] + t["beta"], mean, var, invstd


W2_INPUTS = ("x_q", "x_k", "p1", "W3C", "b3C", "gamma", "beta", "Wa", "ba")
W2_GRADS = dict(xq="x_q", xk="x_k", p1="p1", W3C="W3C", b3C="b3C", gamma="gamma", beta="beta", Wa="Wa", ba="ba")
AGG_GRADS = dict(xv="x_v", p1="p1", W3C="W3C", b3C="b3C", a=None)      # `a`: the weights, or the logits with the softmax inside


def reference_w2(idx, a, eps=EPS, momentum=MOMENTUM, training=True):
    """float64 dict.  training: w2, mean, invstd (as saved for the backward pass), run_mean / run_var (unbiased) / count after nn.BatchNorm1d's update, the nine
    gradients under the loss sum(w2 * g_w2) (keys of W2_GRADS) and the pre-activation z (n, K, C).  Otherwise: w2 and z with a['eval_mean'], a['eval_invstd']."""
    t = _t(a, W2_INPUTS, training)
    ti = torch.from_numpy(idx.astype(np.int64))
    stats = None if training else (torch.tensor(a["eval_mean"], dtype=torch.float64), torch.tensor(a["eval_invstd"], dtype=torch.float64))
    z, mean, var, invstd = _pre_activation(ti, t, eps, stats)
    w2 = torch.relu(z) @ t["Wa"].T + t["ba"]
    res = dict(w2=w2.detach().numpy(), z=z.detach().numpy())
    if not training:
        return res
    (w2 * torch.tensor(a["g_w2"], dtype=torch.float64)).sum().backward()
    rows = idx.size
    res.update(mean=mean.detach().numpy(), invstd=invstd.detach().numpy(), count=COUNT0 + 1,
               run_mean=(1 - momentum) * a["run_mean"].astype(np.float64) + momentum * mean.detach().numpy(),
               run_var=(1 - momentum) * a["run_var"].astype(np.float64) + momentum * var.detach().numpy() * (rows / max(rows - 1, 1)))
    res.update({k: t[src].grad.numpy() for k, src in W2_GRADS.items()})
    return res


def reference_agg(idx, a, softmax):
    """float64 dict: out, the weights (the softmax of a['logits'] over K, or a['weights'] themselves) and the five gradients under sum(out * g_out) (keys of
    AGG_GRADS; `a` is the gradient of the logits with the softmax, of the weights without)"""
    t = _t(a, ("x_v", "p1", "W3C", "b3C", "logits" if softmax else "weights"), True)
    ti = torch.from_numpy(idx.astype(np.int64))
    w = torch.softmax(t["logits"], 1) if softmax else t["weights"]
    out = ((t["x_v"][ti] + (t["p1"] @ t["W3C"].T + t["b3C"])) * w.repeat(1, 1, 8)).sum(1)      # channel c takes weight c % G
    (out * torch.tensor(a["g_out"], dtype=torch.float64)).sum().backward()
    res = dict(out=out.detach().numpy(), weights=w.detach().numpy())
    res.update({k: t[src or ("logits" if softmax else "weights")].grad.numpy() for k, src in AGG_GRADS.items()})
    return res


def min_abs_z(idx, a, eps=EPS):
    """(n, K): per pair the smallest |z| over the channels of the train-mode pre-activation, in float64"""
    with torch.no_grad():
        return _pre_activation(torch.from_numpy(idx.astype(np.int64)), _t(a, W2_INPUTS, False), eps)[0].abs().amin(-1).numpy()


def make_flip_free(idx, a, delta=1e-5, rounds=8, seed=0):
    """moves the scene (a['p1'], in place, float32) until no train-mode pre-activation lies within `delta` of zero in float64: every pair (i, k) with such a
    channel gets U(1e-3, 2e-3) added to p1[i, k, :]; that moves the batch statistics, hence again, at most `rounds` times.  -> the number of pairs touched
    (make_flip_free.rounds: the rounds the last call took).  The caller bounds the touched share (0.1 % of the pairs keeps the scene's distribution)."""
    rng = np.random.default_rng(seed)
    touched = np.zeros(idx.shape, bool)
    for r in range(rounds + 1):
        low = min_abs_z(idx, a)
        bad = low < delta
        if not bad.any():
            break
        assert r < rounds, "still %d pairs within %.0e of a ReLU's edge after %d rounds" % (int(bad.sum()), delta, rounds)
        a["p1"][bad] += rng.uniform(1e-3, 2e-3, (int(bad.sum()), 3)).astype(np.float32)
        touched |= bad
    assert float(low.min()) >= delta
    make_flip_free.rounds = r
    return int(touched.sum())


# ---------------------------------------------------------------------------------------------------------------- the contract
def close(got, ref, what):
    """the project's contract (tests/pointwise_mlp_oracle.close): |got - ref| <= 1e-4 |ref| + 1e-4 max|ref| for EVERY entry; prints and returns the worst
    ratio of an error to its bound"""
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound = 1e-4 * max(float(np.abs(ref).max()), 1e-30) + 1e-4 * np.abs(ref)
    ratio = float((np.abs(got - ref) / bound).max()) if np.isfinite(got).all() else float("inf")
    print("%s: worst error / bound %.4f" % (what, ratio))
    assert ratio <= 1.0, "%s: an entry is off by %.3f times the 1e-4 bound" % (what, ratio)
    return ratio


def small(got, bound, what):
    """a gradient that is exactly 0 in float64 (what the kernel returns is rounding): every entry within `bound` of 0"""
    got = np.asarray(got, np.float64)
    ratio = float(np.abs(got).max()) / bound if np.isfinite(got).all() else float("inf")
    print("%s (0 in float64): worst |entry| / bound %.4f" % (what, ratio))
    assert ratio <= 1.0, "%s: an entry of a zero gradient is %.3f times its bound" % (what, ratio)
    return ratio


# ---------------------------------------------------------------------------------------------------------------- the entries
class HostBackend:
    """numpy buffers for the host-emulated library: 64-byte aligned, or `shift` floats past such a boundary"""
    stream = None

    def put(self, array, shift=0):
        array = np.ascontiguousarray(array)
        raw = np.zeros(array.nbytes + 128, np.uint8)
        off = (-raw.ctypes.data) % 64 + 4 * shift
        out = raw[off:off + array.nbytes].view(array.dtype).reshape(array.shape)
        out[...] = array
        return out

    def fill(self, shape, value, dtype=np.float32):
        return self.put(np.full(shape, value, dtype))

    def ptr(self, buf):
        return None if buf is None else ctypes.c_void_p(buf.ctypes.data)

    def get(self, buf):
        return np.array(buf)


class Entries:
    """the three forward and seven backward entries of attention.hip on one backend.  Outputs are pre-filled with NaN (grad_xk / grad_xv with zeros for the
    scatter entries, which accumulate into them); the workspace has exactly cbl_attn_workspace_bytes bytes.  Every call returns numpy arrays."""

    def __init__(self, lib, backend):
        self.L, self.B = lib, backend
        size_t_results(lib)

    def _call(self, name, *args):
        rc = getattr(self.L, name)(*args, self.B.stream)
        assert rc == 0, "%s returned %d" % (name, rc)

    def _common(self, idx, a, keys, C):
        B, G = self.B, C // 8
        nbytes = self.L.cbl_attn_workspace_bytes(_i(C), _i(G))
        return {k: B.put(a[k]) for k in keys}, B.put(idx), B.fill((nbytes,), 0, np.uint8), _z(nbytes)

    def w2_forward(self, idx, a, training, unaligned=False):
        """unaligned: x_q / x_k start one float into their buffers (not 16-byte aligned: the narrow widths then cannot take the MFMA kernel's float4 loads).
        Evaluation mode: a['eval_mean'] / a['eval_invstd'] go in through the save_* arguments, the BatchNorm buffers are not passed."""
        (n, K), C = idx.shape, a["x_q"].shape[1]
        B, P, G = self.B, self.B.ptr, C // 8
        d, didx, ws, wsn = self._common(idx, a, ("p1", "W3C", "b3C", "gamma", "beta", "Wa", "ba"), C)
        xq, xk = B.put(a["x_q"], int(unaligned)), B.put(a["x_k"], int(unaligned))
        w2 = B.fill((n, K, G), np.nan)
        if training:
            mean, invstd, rm, rv, cnt = B.fill((C,), np.nan), B.fill((C,), np.nan), B.put(a["run_mean"]), B.put(a["run_var"]), B.fill((1,), COUNT0, np.int64)
        else:
            mean, invstd, rm, rv, cnt = B.put(a["eval_mean"]), B.put(a["eval_invstd"]), None, None, None
        self._call("cbl_attn_w2_forward", _i(n), _i(K), _i(C), _i(G), P(xq), P(xk), P(didx), P(d["p1"]), P(d["W3C"]), P(d["b3C"]), P(d["gamma"]), P(d["beta"]),
                   _f(EPS), _f(MOMENTUM), P(rm), P(rv), P(cnt), _i(1 if training else 0), P(d["Wa"]), P(d["ba"]), P(mean), P(invstd), P(w2), P(ws), wsn)
        out = dict(w2=B.get(w2))
        if training:
            out.update(mean=B.get(mean), invstd=B.get(invstd), run_mean=B.get(rm), run_var=B.get(rv), count=int(B.get(cnt)[0]))
        return out

    def agg_forward(self, idx, a, softmax):
        (n, K), C = idx.shape, a["x_v"].shape[1]
        B, P, G = self.B, self.B.ptr, C // 8
        d, didx, _, _ = self._common(idx, a, ("x_v", "p1", "W3C", "b3C", "logits" if softmax else "weights"), C)
        out = B.fill((n, C), np.nan)
        head = (_i(n), _i(K), _i(C), _i(G), P(d["x_v"]), P(didx), P(d["p1"]), P(d["W3C"]), P(d["b3C"]))
        if softmax:
            w = B.fill((n, K, G), np.nan)
            self._call("cbl_attn_agg_softmax_forward", *head, P(d["logits"]), P(w), P(out))
            return dict(out=B.get(out), weights=B.get(w))
        self._call("cbl_attn_agg_forward", *head, P(d["weights"]), P(out))
        return dict(out=B.get(out))

    def _table(self, table):
        """-> the buffers of (order, inv_start, inv_src), which the caller keeps alive over the call"""
        return [None if t is None else self.B.put(t) for t in table]

    def w2_backward(self, idx, a, mean, invstd, table=None):
        """table: None = the scatter entry, else (order or None, inv_start, inv_src) = the gather entry of the width (_csr up to C = 64, _wide_csr above)"""
        (n, K), C = idx.shape, a["x_q"].shape[1]
        B, P, G = self.B, self.B.ptr, C // 8
        d, didx, ws, wsn = self._common(idx, a, ("x_q", "x_k", "p1", "W3C", "b3C", "gamma", "beta", "Wa", "g_w2"), C)
        dm, ds = B.put(np.asarray(mean, np.float32)), B.put(np.asarray(invstd, np.float32))
        shapes = dict(xq=(n, C), xk=(n, C), p1=(n, K, 3), W3C=(C, 3), b3C=(C,), gamma=(C,), beta=(C,), Wa=(G, C), ba=(G,))
        g = {k: B.fill(s, 0.0 if k == "xk" and table is None else np.nan) for k, s in shapes.items()}
        head = [_i(n), _i(K), _i(C), _i(G)] + [P(d[k]) for k in ("x_q", "x_k")] + [P(didx)] + [P(d[k]) for k in ("p1", "W3C", "b3C", "gamma", "beta")]
        head += [P(dm), P(ds), P(d["Wa"]), P(d["g_w2"])]
        name = "cbl_attn_w2_backward" if table is None else "cbl_attn_w2_backward_csr" if C <= 64 else "cbl_attn_w2_backward_wide_csr"
        tab = self._table(table) if table is not None else []
        self._call(name, *head, *[P(t) for t in tab], *[P(g[k]) for k in shapes], P(ws), wsn)
        return {k: B.get(v) for k, v in g.items()}

    def agg_backward(self, idx, a, weights, softmax, table=None):
        """weights: what the forward pass kept (the softmax weights, or the plain weights); the gradient `a` is that of the logits with softmax"""
        (n, K), C = idx.shape, a["x_v"].shape[1]
        B, P, G = self.B, self.B.ptr, C // 8
        d, didx, ws, wsn = self._common(idx, a, ("x_v", "p1", "W3C", "b3C", "g_out"), C)
        dw = B.put(np.asarray(weights, np.float32))
        shapes = dict(xv=(n, C), p1=(n, K, 3), W3C=(C, 3), b3C=(C,), a=(n, K, G))
        g = {k: B.fill(s, 0.0 if k == "xv" and table is None else np.nan) for k, s in shapes.items()}
        head = [_i(n), _i(K), _i(C), _i(G), P(d["x_v"]), P(didx), P(d["p1"]), P(d["W3C"]), P(d["b3C"]), P(dw), P(d["g_out"])]
        outs = [P(g[k]) for k in shapes] + [P(ws), wsn]
        if table is None:
            self._call("cbl_attn_agg_softmax_backward" if softmax else "cbl_attn_agg_backward", *head, *outs)
        else:
            tab = self._table(table)
            self._call("cbl_attn_agg_backward_csr" if C <= 64 else "cbl_attn_agg_backward_wide_csr", *head, *[P(t) for t in tab], *outs, _i(1 if softmax else 0))
        return {k: B.get(v) for k, v in g.items()}


# ---------------------------------------------------------------------------------------------------------------- the checks
def check_w2_forward(got, ref, tag):
    close(got["w2"], ref["w2"], tag + " w2")
    for k in ("mean", "invstd", "run_mean", "run_var"):
        close(got[k], ref[k], tag + " " + k)
    assert got["count"] == ref["count"], (tag, got["count"])


def check_w2_backward(got, ref, tag, gathered):
    n = got["xk"].shape[0]
    for k in W2_GRADS:
        if k == "b3C":                                                 # a bias in front of a train-mode BatchNorm has no gradient
            small(got[k], 1e-4 * float(np.abs(ref["W3C"]).max()), tag + " grad b3C")
        else:
            close(got[k], ref[k], tag + " grad " + k)
    if gathered:
        assert (got["xk"][n - 1] == 0.0).all(), tag + ": the unlisted target's row of grad x_k is not exactly 0"


def check_agg_backward(got, ref, tag, gathered, softmax, g_out):
    n, K = got["a"].shape[:2]
    for k in AGG_GRADS:
        if k == "a" and softmax and K == 1:                            # the softmax of one logit is 1 whatever the logit
            small(got[k], 1e-4 * float(np.abs(g_out).max()), tag + " grad logits")
        else:
            close(got[k], ref[k], tag + " grad " + k)
    if gathered:
        assert (got["xv"][n - 1] == 0.0).all(), tag + ": the unlisted target's row of grad x_v is not exactly 0"


def tables(idx, seed):
    """the gather entries' two tables: targets in index order (no `order`), and in a random processing order"""
    order = np.random.default_rng(seed).permutation(idx.shape[0]).astype(np.int32)
    return {"index order": (None,) + transposed(idx, None), "ordered": (order,) + transposed(idx, order)}


def case(n, K, C, gradients=True):
    """-> (idx, inputs, pairs touched by make_flip_free, its rounds) of the scene a shape is tested on: seeds n + K + C, flip-free where gradients are compared
    (make_flip_free asserts its own limits: the rounds, and no pre-activation within 1e-5 of zero at the end).  The touched share is printed for the log; it is
    C * 2e-5 * the density of z at 0 (about 0.4) per pair — 0.03 % at C = 32, 0.4 % at C = 512 — and asserted where the pairs are many
    (tests/test_attention_oracle_host.py)."""
    seed = n + K + C
    idx, a = neighbours(n, K, seed), scene(n, K, C, seed + 1)
    if not gradients:
        return idx, a, 0, 0
    touched = make_flip_free(idx, a, seed=seed + 2)
    print("scene (%d, %d, %d): make_flip_free touched %d of %d pairs (%.3f %%) in %d rounds" % (n, K, C, touched, n * K, 100.0 * touched / (n * K), make_flip_free.rounds))
    return idx, a, touched, make_flip_free.rounds


def check_all(E, idx, a, tag, unaligned=False):
    """every check of one scene on the entries `E` (the host run; the device file spreads the same calls over its tests)"""
    ref = reference_w2(idx, a)
    check_w2_forward(E.w2_forward(idx, a, True), ref, tag + " train")
    close(E.w2_forward(idx, a, False)["w2"], reference_w2(idx, a, training=False)["w2"], tag + " eval w2")
    if unaligned:
        check_w2_forward(E.w2_forward(idx, a, True, unaligned=True), ref, tag + " train, unaligned rows")
    tabs = tables(idx, idx.size)
    for name, table in [("scatter", None)] + list(tabs.items()):
        check_w2_backward(E.w2_backward(idx, a, ref["mean"], ref["invstd"], table), ref, "%s w2 backward, %s" % (tag, name), table is not None)
    for softmax in (0, 1):
        ra = reference_agg(idx, a, softmax)
        got = E.agg_forward(idx, a, softmax)
        close(got["out"], ra["out"], "%s agg softmax %d out" % (tag, softmax))
        if softmax:
            close(got["weights"], ra["weights"], tag + " agg softmax weights")
        for name, table in [("scatter", None)] + list(tabs.items()):
            check_agg_backward(E.agg_backward(idx, a, ra["weights"], softmax, table), ra, "%s agg backward softmax %d, %s" % (tag, softmax, name),
                               table is not None, softmax, a["g_out"])
