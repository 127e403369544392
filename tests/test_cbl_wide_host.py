"""CPU: the CBL pair kernels (contrastboundary_amd/csrc/cbl_pairs.hip) on feature rows of ANY width — the stage outputs (128 ... 2304 floats), the class
logits (13, 20), widths that are multiples of 4 but not powers of two (12, 48, 72, ...) and widths below 4 — compiled for the HOST and run with wave semantics
(tests/host_emul/wave), through their C entry points, against the oracle's restatement (oracle/cbl_oracle.py point_contrast / tf_contrast): point mask bit
for bit, loss and feature gradient within the kernels' 1e-4 contract.  Both flavours (pytorch heads.py:185-246, TF head.py:462-807 with shadow neighbours,
sample roles and 'labelkl' soft labels), 'softnn' and 'nce', the 'S' margin, and both backward routes: the gather over the transposed neighbour table and
the atomic scatter."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cbl_oracle as C
from tests import oracle_lib as O
from tests.host_emul.host_build import P
from tests.test_cbl_host import host  # noqa: F401  (the fixture that builds and loads the host library)

F = ctypes.c_float

WIDTHS = [1, 3, 12, 13, 20, 48, 68, 72, 96, 128, 200, 256, 512, 2304]
NSAMPLES = [2, 17, 25, 36, 65]
# every width with two neighbour counts, every neighbour count with several widths
GRID = [(d, NSAMPLES[(k + s) % len(NSAMPLES)]) for k, d in enumerate(WIDTHS) for s in (1, 3)]


def placed(shape, misalign=0, dtype=np.float32):
    """a zero array whose data pointer is `misalign` bytes past a 16-byte boundary"""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.zeros(n + 32, np.uint8)
    off = (-raw.ctypes.data) % 16 + misalign
    return raw[off:off + n].view(dtype).reshape(shape)


def transpose(idx, m):
    """the transposed neighbour table (cbl_neighbor_transpose with order = identity): for every target t the pairs p = i * nsample + col (col >= 1) with
    idx[i, col] = t, shadow ids (>= m) left out; inv_src carries one spare entry"""
    ns = idx.shape[1]
    flat = idx.reshape(-1).astype(np.int64)
    p = np.arange(flat.size)
    ok = (flat >= 0) & (flat < m) & (p % ns != 0)
    t, p = flat[ok], p[ok]
    srt = np.argsort(t, kind="stable")
    inv_src = np.concatenate([p[srt], [0]]).astype(np.int32)
    inv_start = np.zeros(m + 1, np.int32)
    inv_start[1:] = np.cumsum(np.bincount(t, minlength=m))
    return inv_start, inv_src


def run_pairs(host, feat, labels, samples, flags, T, weight, ncls=0, kl=0.0, roles=None, valid=None, n_valid=None, misalign=0):
    """forward (+ coefficients and the centre half), then both backward routes -> loss, point_mask, grad (gather route), grad (atomic route)"""
    m, d = feat.shape
    nsample = samples.shape[1]
    n_valid = m if n_valid is None else n_valid
    per_point, mask, stats, loss = np.full(m, np.nan, np.float32), np.full(m, -1, np.int32), np.full(2, np.nan, np.float32), np.full(1, np.nan, np.float32)
    coef, own = np.full((m, nsample), np.nan, np.float32), placed((m, d), misalign)
    own[:] = np.nan
    rc = host.cbl_contrast_pairs_forward_samples(m, n_valid, flags, nsample, d, P(feat), P(labels), ncls, F(kl), P(samples), P(roles), P(valid), None,
                                                 F(T), F(weight), P(per_point), P(mask), P(stats), P(loss), P(coef), P(own), None)
    assert rc == 0, rc
    assert np.isfinite(coef).all() and np.isfinite(own).all()                # every entry written
    one = np.ones(1, np.float32)
    inv_start, inv_src = transpose(samples, m)
    g_gather = placed((m, d), misalign); g_gather[:] = np.nan
    assert host.cbl_contrast_pairs_backward(m, nsample, d, P(feat), P(coef), P(own), None, P(inv_start), P(inv_src), P(stats), P(one), F(weight),
                                            P(g_gather), None) == 0
    g_atomic = placed((m, d), misalign); g_atomic[:] = np.nan
    assert host.cbl_contrast_pairs_backward_atomic(m, n_valid, nsample, d, P(feat), P(coef), P(own), P(samples), P(stats), P(one), F(weight),
                                                   P(g_atomic), None) == 0
    return float(loss[0]), mask, np.array(g_gather), np.array(g_atomic), int(np.diff(inv_start).max())


def check(got_loss, got_mask, grads, rloss, rgrad, rmask, count_mask=False):
    np.testing.assert_array_equal(got_mask > 0 if count_mask else got_mask.astype(bool), rmask)
    assert abs(got_loss - float(rloss)) <= 1e-4 * max(1.0, abs(float(rloss))), (got_loss, float(rloss))
    tol = 1e-4 * max(float(np.abs(rgrad).max()), 1e-30)
    for g in grads:
        np.testing.assert_allclose(g, rgrad, rtol=1e-4, atol=tol)


def scene(n, nsample, d, seed, misalign=0):
    """blocky labels over a unit square (boundaries between them), features spread so that no distance collapses below the TF clamp"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    lab = ((np.floor(xyz[:, 0] * 4) + 4 * np.floor(xyz[:, 1] * 3)).astype(np.int64) % 13).astype(np.int32)
    feat = placed((n, d), misalign)
    feat[:] = rng.normal(size=(n, d)) * (1.5 / np.sqrt(d))
    off = np.int32([n // 3, n])
    idx, _ = O.knnquery(nsample, xyz, xyz, off, off)
    return xyz, feat, lab, np.ascontiguousarray(idx, np.int32)


def points_for(d):
    return 160 if d <= 256 else 64


@pytest.mark.parametrize("d,nsample", GRID)
@pytest.mark.parametrize("nce", [0, 1])
def test_pytorch_flavour(host, d, nsample, nce):
    n, T, weight = points_for(d), 0.7, 0.1
    _, feat, lab, idx = scene(n, nsample, d, seed=7 * d + nsample + nce)
    loss, mask, gg, ga, _ = run_pairs(host, feat, lab, idx, 4 if nce else 0, T, weight)
    rloss, rgrad, rmask = C.point_contrast(np.array(feat), np.eye(13, dtype=np.float32)[lab], idx, temperature=T, weight=weight,
                                           contrast="nce" if nce else "softnn")
    if nsample > 2:
        assert rmask.any()
    check(loss, mask, (gg, ga), rloss, rgrad, rmask, count_mask=bool(nce))


def radius_columns(xyz, nsample, seed):
    """radius-like neighbourhoods: knn columns, a random tail of each row replaced by the shadow index n (tf radius search padding)"""
    n = len(xyz)
    idx, _ = O.knnquery(nsample, xyz, xyz, np.int32([n // 2, n]), np.int32([n // 2, n]))
    keep = np.random.default_rng(seed).integers(max(nsample // 3, 1), nsample + 1, n)
    idx = np.where(np.arange(nsample)[None, :] < keep[:, None], idx, n)
    return np.ascontiguousarray(idx, np.int32)


@pytest.mark.parametrize("d,nsample", GRID)
@pytest.mark.parametrize("contrast,separate", [("softnn", False), ("nce", False), ("softnn", True)])
def test_tf_flavour_with_shadow_neighbours(host, d, nsample, contrast, separate):
    n, T, weight = points_for(d), 0.8, 0.1
    xyz, feat, lab, _ = scene(n, nsample, d, seed=3 * d + nsample)
    lab = lab.copy(); lab[::17] = -1                                      # ignored labels
    idx = radius_columns(xyz, nsample, seed=d)
    if nsample > 2:
        assert (idx == n).any()
    flags = 1 | (4 if contrast == "nce" else 0) | (8 if separate else 0)
    loss, mask, gg, ga, _ = run_pairs(host, feat, lab, idx, flags, T, weight)
    rloss, rgrad, rmask = C.tf_contrast(np.array(feat), lab, idx, temperature=T, weight=weight, contrast=contrast, separate=separate)
    check(loss, mask, (gg, ga), rloss, rgrad, rmask)


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("kl", [False, True])
def test_tf_sample_roles(host, d, kl):
    """sample 'nn2-label-rand6-rand3R' (head.py:560-625: positives, label-mined columns, negatives, negatives unless they hit a neighbour), with hard labels or
    'labelkl' soft labels; shadow neighbours in the label columns"""
    from contrastboundary_amd import heads
    n, k, T, weight = points_for(d), 17, 0.9, 0.1
    xyz, feat, lab, _ = scene(n, k, d, seed=d + 101)
    nbr = radius_columns(xyz, k, seed=d + 5)
    rng = np.random.default_rng(d)
    r1, r2 = rng.integers(0, n, (n, 6)).astype(np.int32), rng.integers(0, n, (n, 3)).astype(np.int32)
    r2[:, 0] = np.minimum(nbr[:, 2], n - 1)
    sample = "nn2-label-rand6-rand3R"
    samples, roles, valid = heads.tf_sample_columns(torch.from_numpy(nbr), sample, rand_idx=[torch.from_numpy(r1), torch.from_numpy(r2)])
    samples, roles, valid = samples.numpy(), roles.numpy(), valid.numpy()
    if kl:
        soft = (0.8 * np.eye(5)[lab % 5] + 0.2 * rng.dirichlet(np.full(5, 0.5), n)).astype(np.float32)   # KL small within a block, large across
        thr = 0.4
        loss, mask, gg, ga, _ = run_pairs(host, feat, soft, samples, 1, T, weight, ncls=5, kl=thr, roles=roles, valid=valid)
        rloss, rgrad, rmask = C.tf_contrast(np.array(feat), soft, nbr, temperature=T, weight=weight, kl_threshold=thr, sample=sample, rand_idx=[r1, r2])
    else:
        lab = lab.copy(); lab[::11] = -1
        loss, mask, gg, ga, _ = run_pairs(host, feat, lab, samples, 1, T, weight, roles=roles, valid=valid)
        rloss, rgrad, rmask = C.tf_contrast(np.array(feat), lab, nbr, temperature=T, weight=weight, sample=sample, rand_idx=[r1, r2])
    assert rmask.any()
    check(loss, mask, (gg, ga), rloss, rgrad, rmask)


@pytest.mark.parametrize("d", [1, 2, 3, 13, 201])
def test_rows_four_byte_aligned(host, d):
    """widths that are not a multiple of 4 are read one dword at a time: a feature / gradient base 4 bytes past a 16-byte boundary is accepted"""
    n, nsample, T, weight = points_for(d), 25, 0.7, 0.1
    _, feat, lab, idx = scene(n, nsample, d, seed=d + 55, misalign=4)
    assert feat.ctypes.data % 16 == 4
    loss, mask, gg, ga, _ = run_pairs(host, feat, lab, idx, 0, T, weight, misalign=4)
    rloss, rgrad, rmask = C.point_contrast(np.array(feat), np.eye(13, dtype=np.float32)[lab], idx, temperature=T, weight=weight)
    check(loss, mask, (gg, ga), rloss, rgrad, rmask)


def test_long_neighbour_lists_of_the_gather(host):
    """targets listed by more than 64 pairs: pass B takes their list 64 entries at a time through the output row"""
    n, nsample, d, T, weight = 200, 65, 72, 0.7, 0.1
    _, feat, lab, idx = scene(n, nsample, d, seed=9)
    idx[:, 1:8] = np.arange(7, dtype=np.int32)[None, :]                   # points 0 ... 6 listed by every point: 200 entries each
    loss, mask, gg, ga, longest = run_pairs(host, feat, lab, idx, 0, T, weight)
    assert longest > 128
    rloss, rgrad, rmask = C.point_contrast(np.array(feat), np.eye(13, dtype=np.float32)[lab], idx, temperature=T, weight=weight)
    check(loss, mask, (gg, ga), rloss, rgrad, rmask)


def test_width_contract(host):
    """any d >= 1 up to CBL_CONTRAST_PAIRS_MAX_D = 4096; rows of d % 4 == 0 floats must be 16-byte aligned, others 4-byte aligned"""
    n, nsample = 8, 3
    idx = np.ascontiguousarray(np.stack([np.arange(n), (np.arange(n) + 1) % n, (np.arange(n) + 2) % n], 1), np.int32)
    lab = (np.arange(n) % 2).astype(np.int32)
    pp, mask, stats, loss = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(2, np.float32), np.zeros(1, np.float32)

    def fwd(d, misalign):
        feat = placed((n, d), misalign)
        return host.cbl_contrast_pairs_forward(n, n, 0, nsample, d, P(feat), P(lab), 0, F(0.0), P(idx), None, F(1.0), F(0.1), P(pp), P(mask), P(stats),
                                               P(loss), None, None, None)
    assert fwd(4096, 0) == 0
    assert fwd(4097, 0) == -3                                             # CBL_ERR_UNSUPPORTED beyond the maximum only
    assert fwd(12, 4) == -1 and fwd(2304, 8) == -1                        # float4 rows: 16-byte alignment
    assert fwd(13, 4) == 0 and fwd(2, 4) == 0
