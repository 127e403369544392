"""TEST ORACLE: ind_max_pool / ind_closest_pool (tensorflow/models/basic_operators.py:155-192) with their gradients, in float64 torch:
    ind_max_pool      torch.cat([x, x.amin(0, keepdim=True)])[inds].amax(1)      (:168-172)
    ind_closest_pool  torch.cat([x, zeros(1, d)])[inds[:, 0]]                    (:189-192; nearest_upsample_block, models/heads/seg_head.py:13-28)
with an id outside [0, n1) read as the shadow row n1.  Gradients by autograd: `amax` / `amin` share the gradient of a maximum / minimum EQUALLY among the
entries that attain it, as tf.reduce_max / tf.reduce_min do.  `restated_max` is the explicit form of that gradient (the contract of cbl_amd.h,
cbl_ind_max_pool_backward_csr), kept as a cross-check of the oracle itself.  TensorFlow is absent, so this is a restatement of the graph code, not a
recording of it.  All comparisons are float equality on elements of x: the tie structure is the same in float32 and float64."""
import functools

import numpy as np
import torch

#        n1,   n2,   k,  d
SHAPES = {"A": (61, 23, 5, 37),        # one-channel kernels; no ties; trailing shadow entries id == n1
          "B": (300, 97, 19, 72),      # float4 path, L = 18, several workgroups and a partial last one; quantised x; repeated ids; ids -1 and n1 + 3
          "C": (40, 12, 4, 8),         # three fully shadow rows; a constant column (nmin = n1); a column whose minimum is attained twice
          "D": (40, 17, 3, 1028),      # two column chunks (257 float4 columns -> 129 + 128 lanes)
          "E": (50, 400, 1, 16),       # upsample shape: 20 source rows nobody references
          "E1": (500, 400, 2, 16),     # closest pool with at most one reference per source row
          "F": (6000, 1500, 38, 144)}  # every pass spans many workgroups; about 40 % shadow entries
QUANTISED = ("B", "D", "F")
SEEDS = {"A": 0, "B": 1, "C": 2, "D": 3, "E": 4, "E1": 5, "F": 6}


def _quantised(rng, n1, d):
    return rng.choice(np.array([0.0, 0.5, 1.0, 1.5], np.float32), size=(n1, d), p=[0.5, 0.2, 0.15, 0.15]).astype(np.float32)


def _trailing_shadow(rng, inds, n1, counts, ids):
    for r, c in enumerate(counts):
        if c:
            inds[r, inds.shape[1] - c:] = rng.choice(ids, size=c)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """-> dict(x (n1, d) f32, inds (n2, k) i32, g (n2, d) f32); unchanged by its users"""
    n1, n2, k, d = SHAPES[name]
    rng = np.random.default_rng(SEEDS[name])
    inds = rng.integers(0, n1, (n2, k)).astype(np.int32)
    if name == "A":
        x = rng.normal(size=(n1, d)).astype(np.float32)
        _trailing_shadow(rng, inds, n1, rng.integers(0, 3, n2), [n1])
    elif name == "B":
        x = _quantised(rng, n1, d)
        few = rng.random(n2) < 0.3                                       # rows left with 1 .. 3 real entries: their maximum can be the column minimum
        _trailing_shadow(rng, inds, n1, np.where(few, rng.integers(k - 3, k, n2), rng.integers(0, 4, n2)), [-1, n1, n1 + 3])
        inds[::5, 1] = inds[::5, 0]                                      # an id twice in a row: counts twice
        inds[3, 0] = -1                                                  # a shadow entry in front of real ones
    elif name == "C":
        x = rng.normal(size=(n1, d)).astype(np.float32)
        x[:, 0] = 0.75
        x[5, 1] = x[9, 1] = x[:, 1].min() - 1.0
        inds[[0, 6, 11]] = n1
        inds[2, 3] = n1
        inds[3, :2] = [5, 9]
    elif name == "D":
        x = _quantised(rng, n1, d)
        _trailing_shadow(rng, inds, n1, rng.integers(0, 3, n2), [n1, -1])
    elif name == "E":
        x = rng.normal(size=(n1, d)).astype(np.float32)
        x[0] = x.min(0) - 1.0                                            # every column minimum sits in row 0, a referenced row
        inds = rng.integers(0, 30, (n2, k)).astype(np.int32)             # rows 30 .. 49: no reference
        inds[0, 0] = 0
        inds[rng.choice(np.arange(1, n2), 25, replace=False), 0] = n1
    elif name == "E1":
        x = rng.normal(size=(n1, d)).astype(np.float32)
        inds[:, 0] = rng.permutation(n1)[:n2]
        inds[rng.choice(n2, 30, replace=False), 0] = n1
    else:
        x = _quantised(rng, n1, d)
        _trailing_shadow(rng, inds, n1, rng.integers(0, int(0.8 * k) + 1, n2), [n1])
    g = rng.normal(size=(n2, d)).astype(np.float32)
    case = dict(x=np.ascontiguousarray(x), inds=np.ascontiguousarray(inds), g=g, name=name)
    for a in (case["x"], case["inds"], case["g"]):
        a.setflags(write=False)
    return case


def _row_ids(inds, n1):
    inds = torch.tensor(np.asarray(inds), dtype=torch.int64)
    return torch.where((inds >= 0) & (inds < n1), inds, torch.full_like(inds, n1))


@functools.lru_cache(maxsize=None)
def reference_max(name):
    """-> out (n2, d), grad_x (n1, d) float64 numpy, by autograd of the composition"""
    case = make_case(name)
    x = torch.tensor(case["x"], dtype=torch.float64, requires_grad=True)
    out = torch.cat([x, x.amin(0, keepdim=True)])[_row_ids(case["inds"], x.shape[0])].amax(1)
    out.backward(torch.tensor(case["g"], dtype=torch.float64))
    return out.detach().numpy(), x.grad.numpy()


@functools.lru_cache(maxsize=None)
def reference_closest(name):
    case = make_case(name)
    x = torch.tensor(case["x"], dtype=torch.float64, requires_grad=True)
    out = torch.cat([x, torch.zeros_like(x[:1])])[_row_ids(case["inds"], x.shape[0])[:, 0]]
    out.backward(torch.tensor(case["g"], dtype=torch.float64))
    return out.detach().numpy(), x.grad.numpy()


def ties(case):
    """-> shadow (d), out (n2, d), cnt (n2, d), nsh (n2, d) = the row's shadow entries that attain its maximum; float64 / int"""
    x = case["x"].astype(np.float64)
    n1 = x.shape[0]
    ids = _row_ids(case["inds"], n1).numpy()
    shadow = x.min(0)
    v = np.concatenate([x, shadow[None]])[ids]                          # (n2, k, d)
    out = v.max(1)
    hit = v == out[:, None]
    return shadow, out, hit.sum(1), (hit & (ids == n1)[..., None]).sum(1)


def restated_max(case):
    """the explicit gradient (cbl_amd.h): -> out, grad_x float64"""
    x = case["x"].astype(np.float64)
    n1 = x.shape[0]
    ids = _row_ids(case["inds"], n1).numpy()
    shadow, out, cnt, nsh = ties(case)
    w = case["g"].astype(np.float64) / cnt
    S = (w * nsh).sum(0)
    nmin = (x == shadow).sum(0)
    grad = np.zeros_like(x)
    for r in range(ids.shape[0]):
        for j in range(ids.shape[1]):
            s = ids[r, j]
            if s < n1:
                grad[s] += (x[s] == out[r]) * w[r]
    return out, grad + (x == shadow) * (S / nmin)


def assert_tied(case):
    """the precondition that makes a quantised case meaningful: at least 10 % of the (r, c) share their maximum, at least one with a shadow entry"""
    _, _, cnt, nsh = ties(case)
    assert (cnt > 1).mean() >= 0.10, "bad seed: only %.3f of the maxima are tied" % (cnt > 1).mean()
    assert ((nsh > 0) & (cnt > nsh)).any(), "bad seed: no maximum shared between a real entry and a shadow entry"


def close(got, ref, what=""):
    """the project's contract: 1e-4 relative, 1e-4 * max|ref| absolute (as tests/pointwise_mlp_oracle.close)"""
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4 * max(float(np.abs(ref).max()), 1e-30), err_msg=what)
