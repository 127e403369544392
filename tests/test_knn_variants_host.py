"""CPU: the tie policies and derived forms of the K-nearest-neighbour search (contrastboundary_amd/csrc/knn_grid.hip, knn_exact.hip, knn_dispatch.hip;
/root/reference/pytorch/lib/pointops/src/knnquery/knnquery_cuda_kernel.cu:65-111) run from the host build of the whole library (tests/host_emul/full_library.py,
wave semantics) through their C entry points, on a cloud with a lattice patch (exactly tied distances) against the oracle (oracle/pointops_oracle.c) and
brute force in numpy:
    cbl_knnquery_set      the reference's neighbour SET per query, its distances bit for bit, its column 0
    cbl_knnquery_anytie   the K smallest by (distance, index) — a rule of its own, stated in numpy here
    cbl_knnquery_ordered  any policy + the cell order of the supports (a permutation, cloud by cloud)
    cbl_knnquery_prefix   a K = 16 table derived from a K = 36 one = the K = 16 search, bit for bit, ties included
    cbl_knn_grid_block_candidates, cbl_knn_indices_to_local (tensorflow/ops/nearest_neighbors/knn_.cxx:104-135: local int64 indices of a dense batch)"""
import ctypes

import numpy as np
import pytest

from tests import oracle_lib as O
from tests.host_emul import full_library
from tests.host_emul.host_build import P, size_t_results
from tests.test_knn_host import cloud


@pytest.fixture(scope="module")
def host():
    return size_t_results(full_library.load())


def scene():
    xyz = np.concatenate([cloud("lattice", 2200, 31), cloud("uniform", 400, 32) + 2.5])
    return np.ascontiguousarray(xyz, np.float32), np.int32([2200, 2600])


def search(host, entry, K, xyz, off, extra=()):
    n, b = xyz.shape[0], len(off)
    idx, d2 = np.full((n, K), -7, np.int32), np.full((n, K), np.nan, np.float32)
    nbytes = host.cbl_knnquery_workspace_bytes(b, n, n, K)
    ws = np.zeros(nbytes + 64, np.uint8)
    rc = getattr(host, entry)(b, n, n, K, P(xyz), P(xyz), P(off), P(off), P(idx), P(d2), *extra, P(ws), ctypes.c_size_t(nbytes), None)
    assert rc == 0, (entry, rc)
    return idx, d2, ws, nbytes


def brute(xyz, off, K):
    """the K smallest by (distance, index) per query inside its cloud, with the kernels' distance expression"""
    out = np.zeros((len(xyz), K), np.int32)
    d2o = np.zeros((len(xyz), K), np.float32)
    s = 0
    for e in off:
        p = xyz[s:e]
        d = p[:, None, :] - p[None, :, :]
        d2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float32)
        order = np.lexsort((np.broadcast_to(np.arange(e - s), d2.shape), d2), axis=-1)[:, :K]
        out[s:e] = order + s
        d2o[s:e] = np.take_along_axis(d2, order, 1)
        s = e
    return out, d2o


@pytest.mark.parametrize("K", [16, 36])
def test_tie_policies(host, K):
    xyz, off = scene()
    ridx, rd2 = O.knnquery(K, xyz, xyz, off, off)
    tied = (np.diff(rd2, axis=1) == 0).any(1)
    assert tied.sum() > 20                                             # the lattice patch: rows with exactly equal distances
    idx, d2, _, _ = search(host, "cbl_knnquery_set", K, xyz, off)
    np.testing.assert_array_equal(d2.view(np.uint32), rd2.view(np.uint32))
    np.testing.assert_array_equal(idx[:, 0], ridx[:, 0])
    np.testing.assert_array_equal(np.sort(idx, 1), np.sort(ridx, 1))
    np.testing.assert_array_equal(idx[~tied], ridx[~tied])
    idx, d2, _, _ = search(host, "cbl_knnquery_anytie", K, xyz, off)
    bidx, bd2 = brute(xyz, off, K)
    np.testing.assert_array_equal(d2.view(np.uint32), rd2.view(np.uint32))
    np.testing.assert_array_equal(d2.view(np.uint32), bd2.view(np.uint32))
    np.testing.assert_array_equal(idx, bidx)


def test_cell_order_and_the_candidate_count(host):
    xyz, off = scene()
    n, K = len(xyz), 16
    ridx, rd2 = O.knnquery(K, xyz, xyz, off, off)
    for policy in (0, 2):
        cell = np.full(n, -1, np.int32)
        idx, d2, ws, nbytes = search(host, "cbl_knnquery_ordered", K, xyz, off, extra=(policy, P(cell)))
        np.testing.assert_array_equal(d2.view(np.uint32), rd2.view(np.uint32))
        if policy == 0:
            np.testing.assert_array_equal(idx, ridx)
        np.testing.assert_array_equal(np.sort(cell), np.arange(n))     # a permutation of the supports
        assert cell[:2200].max() < 2200 and cell[2200:].min() >= 2200   # clouds one after the other
        # cell by cell: consecutive entries are near each other far more often than a random order would have them
        step = np.linalg.norm(xyz[cell[1:2200]] - xyz[cell[:2199]], axis=1)
        assert np.median(step) < 0.25 * np.median(np.linalg.norm(xyz[1:2200] - xyz[:2199], axis=1))
    count = np.full(n, -1, np.int32)
    assert host.cbl_knn_grid_block_candidates(len(off), n, K, P(off), P(count), P(ws), ctypes.c_size_t(nbytes), None) == 0
    assert count.min() >= 1 and count[:2200].max() <= 2200 and count[2200:].max() <= 400
    assert count[:2200].mean() < 0.5 * 2200                           # the point of the grid: a fraction of the brute-force pairs


@pytest.mark.parametrize("policy", [0, 1])
def test_narrow_table_derived_from_a_wide_one(host, policy):
    xyz, off = scene()
    n, b = len(xyz), len(off)
    wide, dw, _, _ = search(host, "cbl_knnquery" if policy == 0 else "cbl_knnquery_set", 36, xyz, off)
    r16, rd16 = O.knnquery(16, xyz, xyz, off, off)
    idx, d2 = np.full((n, 16), -7, np.int32), np.full((n, 16), np.nan, np.float32)
    nbytes = host.cbl_knnquery_prefix_workspace_bytes(n)
    ws = np.zeros(nbytes + 64, np.uint8)
    rc = host.cbl_knnquery_prefix(b, n, n, 36, 16, P(xyz), P(xyz), P(off), P(off), P(wide), P(dw), P(idx), P(d2), policy, P(ws), ctypes.c_size_t(nbytes), None)
    assert rc == 0
    np.testing.assert_array_equal(d2.view(np.uint32), rd16.view(np.uint32))
    if policy == 0:
        np.testing.assert_array_equal(idx, r16)
    else:
        np.testing.assert_array_equal(np.sort(idx, 1), np.sort(r16, 1)); np.testing.assert_array_equal(idx[:, 0], r16[:, 0])


def test_local_indices_of_a_dense_batch(host):
    B, M, K, N = 3, 50, 8, 400
    rng = np.random.default_rng(0)
    idx = np.stack([rng.integers(0, N, (M, K)) + bi * N for bi in range(B)]).astype(np.int32)
    out = np.full((B, M, K), -1, np.int64)
    assert host.cbl_knn_indices_to_local(B, M, K, N, P(idx), P(out), None) == 0
    np.testing.assert_array_equal(out, idx.astype(np.int64) - (np.arange(B) * N)[:, None, None])
